// bigsi_kernels.hpp -- CDNA4 (gfx950) device code of the BIGSI query hot path.
//
// Data layout in HBM: the index is m rows x stride_words uint64 (stride a multiple of 16 words = 128 B).
// A row holds exactly the reference's row bytes (bitarray.tobytes(), bigsi/storage/base.py:85-99), so a
// little-endian uint64 load of word w covers columns [64w, 64w+64) with column c at bit
// ((c>>3)&7)*8 + 7-(c&7).  AND / popcount / bit-sliced addition are agnostic to that permutation; it is
// only applied where set bits become colour ids (compaction, counter expansion).
//
// Kernels: K1 k_kmer_insert/resolve/rank/rows, K2/K3a k_and_exact, K2/K3b k_and_count,
// K4 k_rank_select / k_hits_totals / k_hits_write, K5 k_presence, plus lookup / storage / build helpers.
// All bitwise, HBM-bound work: no MFMA.  Wavefront = 64 lanes everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bigsi_launch.hpp"      // kBlock, kVec, kLdsMaxPos: shared with the host's launch rule
#include "bigsi_score.hpp"
#include "bigsi_device.hpp"     // the small device helpers, MurmurHash3 and row_of_hash: shared with bigsi_kmercount_kernels.hpp

namespace bigsi {

constexpr uint32_t kEmpty = 0xFFFFFFFFu;

// block-wide exclusive scan of one uint32 per thread (blockDim.x a multiple of 64, up to 1024); returns prefix,
// *total = block sum.
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *total, uint32_t *lds /* >= blockDim.x/64 entries */)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // inclusive scan of the wavefront on the DPP path (shifts within rows of 16 lanes, then the row broadcasts): seven VALU adds instead
    // of six round trips through the LDS crossbar (__shfl_up = ds_bpermute) -- it is on the chain of every latency-bound call
    uint32_t incl = v;
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x111, 0xf, 0xf, false);      // row_shr:1
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x112, 0xf, 0xf, false);      // row_shr:2
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x114, 0xf, 0xf, false);      // row_shr:4
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x118, 0xf, 0xf, false);      // row_shr:8
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x142, 0xa, 0xf, false);      // row_bcast:15 into rows 1 and 3
    incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, 0x143, 0xc, 0xf, false);      // row_bcast:31 into rows 2 and 3
    __syncthreads();   // protect lds reuse across calls
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    uint32_t base = 0, tot = 0;
    const uint32_t nw = blockDim.x >> 6;
    for (uint32_t w = 0; w < nw; w++) {
        uint32_t x = lds[w];
        if (w < wave) base += x;
        tot += x;
    }
    *total = tot;
    return base + incl - v;
}

// the same for a FLAG per thread (0 / 1): the wavefront's part is a ballot and two mbcnt instead of six cross-lane shuffles (1.0 us
// of a single query's K1 was the scan above).  No barrier after the LDS reads: the caller reuses `lds` only behind one of its own.
__device__ __forceinline__ uint32_t block_exclusive_scan_flag(bool flag, uint32_t *total, uint32_t *lds /* >= blockDim.x/64 entries */)
{
    const uint64_t bal = __ballot(flag);
    const uint32_t in_wave = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
    const uint32_t wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63u) == 0) lds[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t base = 0, tot = 0;
    for (uint32_t w = 0; w < nw; w++) {
        const uint32_t x = lds[w];
        base += w < wave ? x : 0u;
        tot += x;
    }
    *total = tot;
    return base + in_wave;
}

// ------------------------------------------------------------------------------ K1: k-merise + dedupe + hash
// Restates, per query sequence:
//   seq_to_kmers (bigsi/utils/fncts.py:63-65)          every window of k bytes, no validation;
//   set(kmers) (bigsi/graph/index.py:45, graph/bigsi.py:179)  unique *query strings* (a k-mer and its reverse
//                                                       complement are two), kept in first-occurrence order;
//   canonical + generate_hashes (fncts.py:51-54, bloom/bloomfilter.py:5-13, graph/index.py:62-70)
//                                                       h row ids per unique k-mer, seeds 0..h-1;
//   min_kmers = ceil(u * threshold) (graph/bigsi.py:179) in IEEE double, as Python evaluates it.
// Four launches, the three string-heavy ones with ONE THREAD PER K-MER POSITION of the whole batch (a 256 x 1 kbp batch
// is 248k positions: the chip is full, where one workgroup per query left 252 of 256 CUs with 4 waves each):
//   K1a k_kmer_insert   open-addressing table of positions per query (global scratch), keyed by string equality; the
//                       slot converges to the smallest position of its class (deterministic whatever the atomics' order)
//   K1b k_kmer_resolve  every position reads its class representative
//   K1c k_kmer_rank     one workgroup per query: ordered compaction of representatives -> unique index, u, min_kmers
//   K1d k_kmer_rows     representatives: canonical form, MurmurHash3 with seeds 0..h-1, floor-mod m -> row ids
struct PosRef {
    uint32_t q, i;
    const char *s;
};
__device__ __forceinline__ PosRef locate(uint64_t p, const uint32_t *__restrict__ pos_query, const uint64_t *__restrict__ pos_off,
                                         const char *__restrict__ seqs, const uint64_t *__restrict__ seq_off)
{
    const uint32_t q = pos_query[p];
    return PosRef{q, (uint32_t)(p - pos_off[q]), seqs + seq_off[q]};
}

__device__ __forceinline__ uint32_t fnv1a(const char *s, uint32_t k)
{
    uint32_t h = 2166136261u;
    for (uint32_t j = 0; j < k; j++) h = (h ^ (uint8_t)s[j]) * 16777619u;
    return h ^ (h >> 15);
}

// Compile-time k (KF = 31, the reference's default k, bigsi/constants.py:13): the window is loaded once into registers
// with KF independent byte loads and everything after that (dedupe hash, canonical choice, MurmurHash3 x h) is
// straight-line register code.  KF = 0 is the generic run-time-k path.
template <int KF>
struct RegKmer {
    uint32_t f[KF > 0 ? KF : 1];      // one register per byte (a uint8_t array would live in scratch)
    __device__ __forceinline__ void load(const char *s)
    {
#pragma unroll
        for (int j = 0; j < KF; j++) f[j] = (uint8_t)s[j];
    }
    __device__ __forceinline__ uint32_t fnv() const
    {
        uint32_t h = 2166136261u;
#pragma unroll
        for (int j = 0; j < KF; j++) h = (h ^ f[j]) * 16777619u;
        return h ^ (h >> 15);
    }
    // canonical form packed into little-endian words (utils/fncts.py:51-54)
    __device__ __forceinline__ void canonical_words(uint32_t (&w)[(KF + 3) / 4 > 0 ? (KF + 3) / 4 : 1]) const
    {
        // lexicographic compare of the k-mer with its reverse complement, first difference decides; select-only code
        uint32_t rc = 0, decided = 0;
#pragma unroll
        for (int j = 0; j < KF; j++) {
            const uint32_t a = f[j], b = complement((uint8_t)f[KF - 1 - j]);
            const uint32_t take = (decided ^ 1u) & (uint32_t)(a != b);
            rc = take ? (uint32_t)(b < a) : rc;
            decided |= take;
        }
#pragma unroll
        for (int i = 0; i < (KF + 3) / 4; i++) w[i] = 0;
#pragma unroll
        for (int j = 0; j < KF; j++) {
            const uint32_t c = rc ? (uint32_t)complement((uint8_t)f[KF - 1 - j]) : f[j];
            w[j >> 2] |= (uint32_t)c << (8 * (j & 3));
        }
    }
};

// MurmurHash3_x86_32 over KF bytes already packed in words (tail bytes in the low bits of the last word)
template <int KF>
__device__ __forceinline__ uint32_t murmur3_words(const uint32_t *w, uint32_t seed)
{
    const uint32_t c1 = 0xcc9e2d51u, c2 = 0x1b873593u;
    uint32_t h1 = seed;
#pragma unroll
    for (int i = 0; i < KF / 4; i++) {
        uint32_t k1 = w[i];
        k1 *= c1; k1 = rotl32(k1, 15); k1 *= c2;
        h1 ^= k1; h1 = rotl32(h1, 13); h1 = h1 * 5u + 0xe6546b64u;
    }
    if (KF & 3) {
        uint32_t k1 = w[KF / 4];
        k1 *= c1; k1 = rotl32(k1, 15); k1 *= c2; h1 ^= k1;
    }
    h1 ^= (uint32_t)KF;
    h1 ^= h1 >> 16; h1 *= 0x85ebca6bu; h1 ^= h1 >> 13; h1 *= 0xc2b2ae35u; h1 ^= h1 >> 16;
    return h1;
}

__device__ __forceinline__ bool kmer_equal(const char *a, const char *b, uint32_t k)
{
    for (uint32_t j = 0; j < k; j++)
        if (a[j] != b[j]) return false;
    return true;
}


// ---- 31-mers on packed words (k_reads_fused, k_kmerize_lds<31>).  The sequence is staged in LDS as 32-bit words (`sw`), its
// byte-wise complement (utils/fncts.py:12) likewise, 4 pad bytes in front (`cw`): a k-mer is eight words cut out with
// v_alignbyte, its reverse complement the complement string read backwards, and the lexicographic comparison of
// utils/fncts.py:51-54 an eight-word big-endian compare -- about 75 vector operations where the byte-wise form takes 450.
__device__ __forceinline__ void kmer31_words(const uint32_t *sw, uint32_t p, uint32_t (&wf)[8])
{
    uint32_t d[9];
#pragma unroll
    for (int i = 0; i < 9; i++) d[i] = sw[(p >> 2) + i];
#pragma unroll
    for (int i = 0; i < 8; i++) wf[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], p & 3u);
    wf[7] &= 0x00ffffffu;                                   // little-endian words, the last one holds 3 bytes
}

// equal k-mers have equal fingerprints; a match is always verified on the bytes / words
__device__ __forceinline__ uint32_t kmer31_fingerprint(const uint32_t (&wf)[8])
{
    uint32_t fp = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) fp = (fp ^ wf[i]) * 0x9E3779B1u;
    return fp ^ (fp >> 15);
}

// canonical form (the smaller of k-mer and reverse complement) and MurmurHash3_x86_32's per-word mix of it, which does
// not depend on the seed: k1[0..6] full blocks, k1[7] the 3-byte tail
__device__ __forceinline__ void kmer31_canonical_premix(const uint32_t (&wf)[8], const uint32_t *cw, uint32_t p, uint32_t (&k1)[8])
{
    // x[i] = complement bytes p+27-4i .. p+30-4i as one little-endian word = bytes 4i .. 4i+3 of the reverse complement with
    // the FIRST in the top byte (the last word: 3 bytes + a zero)
    uint32_t e[9], x[8];
    const uint32_t base = ((p + 31u) >> 2) - 7u, sh = (p + 3u) & 3u;
#pragma unroll
    for (int i = 0; i < 9; i++) e[i] = cw[base + i];
#pragma unroll
    for (int i = 0; i < 8; i++) x[i] = __builtin_amdgcn_alignbyte(e[8 - i], e[7 - i], sh);
    x[7] &= 0xffffff00u;
    bool rc = false, decided = false;                      // reverse complement < k-mer ?
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint32_t f = __builtin_bswap32(wf[i]);
        const bool ne = f != x[i];
        rc = (!decided && ne) ? x[i] < f : rc;
        decided = decided || ne;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t w = rc ? __builtin_bswap32(x[i]) : wf[i];
        w *= 0xcc9e2d51u; w = rotl32(w, 15); w *= 0x1b873593u;
        k1[i] = w;
    }
}

__device__ __forceinline__ uint32_t murmur3_31_finish(const uint32_t (&k1)[8], uint32_t seed)
{
    uint32_t h1 = seed;
#pragma unroll
    for (int i = 0; i < 7; i++) { h1 ^= k1[i]; h1 = rotl32(h1, 13); h1 = h1 * 5u + 0xe6546b64u; }
    h1 ^= k1[7];                                           // the 3 tail bytes
    h1 ^= 31u;
    h1 ^= h1 >> 16; h1 *= 0x85ebca6bu; h1 ^= h1 >> 13; h1 *= 0xc2b2ae35u; h1 ^= h1 >> 16;
    return h1;
}

template <int KF>
__global__ __launch_bounds__(kBlock) void k_kmer_insert(
    const char *__restrict__ seqs, const uint64_t *__restrict__ seq_off, const uint64_t *__restrict__ pos_off,
    const uint32_t *__restrict__ pos_query, const uint64_t *__restrict__ tab_off, uint32_t *__restrict__ tab,
    uint32_t k, uint64_t total_pos, uint32_t *__restrict__ hsh)
{
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= total_pos) return;
    const PosRef r = locate(p, pos_query, pos_off, seqs, seq_off);
    uint32_t *t = tab + tab_off[r.q];
    const uint32_t mask = (uint32_t)(tab_off[r.q + 1] - tab_off[r.q]) - 1u;   // table size: power of two >= 2n
    uint32_t hv;
    if (KF > 0) {
        RegKmer<KF> km;
        km.load(r.s + r.i);
        hv = km.fnv();
    } else {
        hv = fnv1a(r.s + r.i, k);
    }
    hsh[p] = hv;
    uint32_t slot = hv & mask;
    for (;;) {
        const uint32_t cur = atomicCAS(&t[slot], kEmpty, r.i);
        if (cur == kEmpty) break;
        if (kmer_equal(r.s + cur, r.s + r.i, k)) { atomicMin(&t[slot], r.i); break; }
        slot = (slot + 1) & mask;
    }
}

__global__ __launch_bounds__(kBlock) void k_kmer_resolve(
    const char *__restrict__ seqs, const uint64_t *__restrict__ seq_off, const uint64_t *__restrict__ pos_off,
    const uint32_t *__restrict__ pos_query, const uint64_t *__restrict__ tab_off, const uint32_t *__restrict__ tab,
    uint32_t k, uint64_t total_pos, const uint32_t *__restrict__ hsh, uint32_t *__restrict__ rep)
{
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= total_pos) return;
    const PosRef r = locate(p, pos_query, pos_off, seqs, seq_off);
    const uint32_t *t = tab + tab_off[r.q];
    const uint32_t mask = (uint32_t)(tab_off[r.q + 1] - tab_off[r.q]) - 1u;
    uint32_t slot = hsh[p] & mask;
    uint32_t c;
    for (;;) {
        c = t[slot];      // the table is final: written by the previous launch
        if (c == r.i || kmer_equal(r.s + c, r.s + r.i, k)) break;
        slot = (slot + 1) & mask;
    }
    rep[p] = c;
}

__global__ __launch_bounds__(kBlock) void k_kmer_rank(
    const uint64_t *__restrict__ seq_off, const uint64_t *__restrict__ pos_off, const uint32_t *__restrict__ rep,
    uint32_t k, double threshold, uint32_t *__restrict__ first_pos, uint32_t *__restrict__ uidx, uint32_t *__restrict__ pos_unique,
    uint32_t *__restrict__ num_kmers, uint32_t *__restrict__ num_unique, uint32_t *__restrict__ min_kmers)
{
    __shared__ uint32_t lds[16];
    const uint32_t q = blockIdx.x;
    const uint64_t len = seq_off[q + 1] - seq_off[q];
    const uint32_t n = len >= k ? (uint32_t)(len - k + 1) : 0u;
    const uint64_t P = pos_off[q];
    const uint32_t *rp = rep + P;
    uint32_t *fp = first_pos + P, *ux = uidx + P, *pu = pos_unique + P;
    uint32_t u = 0;
    for (uint32_t base = 0; base < n; base += kBlock) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t flag = (i < n && rp[i] == i) ? 1u : 0u;
        uint32_t tot;
        const uint32_t pre = block_exclusive_scan(flag, &tot, lds);
        if (flag) { fp[u + pre] = i; ux[i] = u + pre; }
        u += tot;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += kBlock) pu[i] = ux[rp[i]];   // position -> its unique k-mer (graph/bigsi.py:233)
    if (threadIdx.x == 0) {
        num_kmers[q] = n;
        num_unique[q] = u;
        const double mk = ceil((double)u * threshold);      // one IEEE multiply, as Python's int * float
        min_kmers[q] = mk > 0.0 ? (uint32_t)mk : 0u;          // counts are >= 0, so a negative bound behaves like 0
    }
}

template <int KF>
__global__ __launch_bounds__(kBlock) void k_kmer_rows(
    const char *__restrict__ seqs, const uint64_t *__restrict__ seq_off, const uint64_t *__restrict__ pos_off,
    const uint32_t *__restrict__ pos_query, const uint32_t *__restrict__ rep, const uint32_t *__restrict__ uidx,
    uint32_t k, uint32_t h, uint64_t m, uint64_t total_pos, uint64_t *__restrict__ rows)
{
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= total_pos) return;
    const PosRef r = locate(p, pos_query, pos_off, seqs, seq_off);
    if (rep[p] != r.i) return;        // duplicates of an earlier window contribute nothing
    const char *km = r.s + r.i;
    uint64_t *dst = rows + (pos_off[r.q] + uidx[p]) * h;
    if (KF > 0) {
        RegKmer<KF> reg;
        reg.load(km);
        uint32_t w[(KF + 3) / 4 > 0 ? (KF + 3) / 4 : 1];
        reg.canonical_words(w);
        for (uint32_t sd = 0; sd < h; sd++) dst[sd] = row_of_hash(murmur3_words<KF>(w, sd), m);
    } else {
        const KmerView v{km, k, use_revcomp(km, k)};
        for (uint32_t sd = 0; sd < h; sd++) dst[sd] = row_of_hash(murmur3_32(v, sd), m);
    }
}

// K1 fused: ONE launch for batches whose longest query has at most kLdsMaxPos k-mer positions (a 4 kbp query; reads
// and gene-length queries).  One workgroup per query; the sequence and the dedupe table live in LDS (ds_cmpst / ds_min
// instead of L2 atomics), and the workgroup goes insert -> resolve -> ordered compaction -> hash without leaving the CU.
// Same results as the four-kernel path above, which remains the route for longer queries.

// The bytes of ONE query passed BY VALUE in the kernel arguments (a one-call search of a single sequence).  The runtime writes a
// launch's arguments into device-visible memory together with the packet, so the kernel's first loads are local instead of a round
// trip over the host link: scripts/probe/latency_probe.hip, 1 KB read by one workgroup + flag: 15.1 us from pinned memory (E),
// 9.9 us from the arguments (M); every KB of arguments costs the launch about 1 us, hence two sizes.
template <int N>
struct SeqArg {
    uint32_t w[N / 4];
};
template <>
struct SeqArg<0> {
};
constexpr uint32_t kSeqArgSmall = 1024, kSeqArgLarge = 3072, kSeqArgRead = 96;

template <int KF>
__device__ __forceinline__ uint32_t dedupe_hash(const char *km, uint32_t k)
{
    if (KF > 0) {
        RegKmer<KF> r;
        r.load(km);
        return r.fnv();
    }
    return fnv1a(km, k);
}

// the h rows of the k-mer at position i of a query staged in LDS (sq: its bytes; sc: KF == 31, their complements behind 4 pad bytes)
template <int KF>
// (seeds [sd0, sd1) only: dst[sd] for those)
__device__ __forceinline__ void kmer_rows(const char *sq, const char *sc, uint32_t i, uint32_t k, uint32_t sd0, uint32_t sd1, uint64_t m, uint64_t *dst)
{
    if (KF == 31) {
        uint32_t wf[8], k1[8];
        kmer31_words(reinterpret_cast<const uint32_t *>(sq), i, wf);
        kmer31_canonical_premix(wf, reinterpret_cast<const uint32_t *>(sc), i, k1);
        for (uint32_t sd = sd0; sd < sd1; sd++) dst[sd] = row_of_hash(murmur3_31_finish(k1, sd), m);
    } else if (KF > 0) {
        RegKmer<KF> reg;
        reg.load(sq + i);
        uint32_t w[(KF + 3) / 4 > 0 ? (KF + 3) / 4 : 1];
        reg.canonical_words(w);
        for (uint32_t sd = sd0; sd < sd1; sd++) dst[sd] = row_of_hash(murmur3_words<KF>(w, sd), m);
    } else {
        const KmerView v{sq + i, k, use_revcomp(sq + i, k)};
        for (uint32_t sd = sd0; sd < sd1; sd++) dst[sd] = row_of_hash(murmur3_32(v, sd), m);
    }
}

template <int KF, int ARGB = 0 /* > 0: the one sequence of the batch is `sarg` (ARGB bytes of kernel arguments), not seqs */>
__global__ __launch_bounds__(1024) void k_kmerize_lds(
    const char *__restrict__ seqs, const uint64_t *__restrict__ seq_off, const uint64_t *__restrict__ pos_off,
    uint32_t k, uint32_t h, uint64_t m, double threshold, uint32_t tab_cap, uint32_t tab_mult, uint32_t hs_cap, uint32_t sq_bytes /* multiple of 16 */, uint32_t *__restrict__ first_pos,
    uint32_t *__restrict__ uidx, uint32_t *__restrict__ pos_unique, uint32_t *__restrict__ rep_out, uint64_t *__restrict__ rows,
    uint32_t *__restrict__ num_kmers, uint32_t *__restrict__ num_unique, uint32_t *__restrict__ min_kmers,
    uint64_t *__restrict__ rows_sorted /* non-null: also emit the query's row list in address order (what k_sort_rows does) */,
    uint64_t *__restrict__ preset /* non-null: the query's `preset_words` result words are set to preset_value here -- what the sliced
                                     (latency-bound) row-AND launches combine into with atomics; saves a memset launch per call */,
    uint64_t preset_words, uint64_t preset_value,
    uint64_t *__restrict__ pos_off_out /* non-null: seqs / seq_off / pos_off are read straight from pinned host memory (a one-call
                                          search: no upload); the device copy of pos_off the later kernels read is written here */,
    uint32_t one_len /* > 0: the batch is ONE sequence of this length (its offset tables need not be read: a PCIe round trip less) */,
    uint32_t parts /* workgroups per query, a power of two (gridDim.x = queries * parts).  > 1 -- a handful of queries whose positions fit one pass of
                      the workgroup (n <= blockDim.x), no sorted copy: every part dedupes the whole query (same table, same ranks: the
                      representative of a k-mer is its smallest position whatever the order of the inserts), then hashes and writes
                      only its share of the unique k-mers.  One CU takes 4 us to hash the ~970 k-mers of a 1 kbp query for 4 seeds
                      (profiles/r05_k1_phases.txt): that part of a latency-bound call is ALU work, and this spreads it over `parts` CUs */,
    const SeqArg<ARGB> sarg)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t q = blockIdx.x / parts, part = blockIdx.x - q * parts, n_queries = gridDim.x / parts;
    if (pos_off_out && threadIdx.x == 0 && part == 0) {
        if (one_len) {
            pos_off_out[0] = 0;
            pos_off_out[1] = one_len >= k ? one_len - k + 1 : 0u;
        } else {
            pos_off_out[q] = pos_off[q];
            if (q + 1 == n_queries) pos_off_out[n_queries] = pos_off[n_queries];
        }
    }
    if (preset && part == 0) {
        uint64_t *pq = preset + (uint64_t)q * preset_words;
        for (uint64_t i = threadIdx.x; i < preset_words; i += blockDim.x) pq[i] = preset_value;
    }
    uint32_t *tab = reinterpret_cast<uint32_t *>(smem);
    uint32_t *scan = tab + tab_cap + tab_cap / 32 + 4;   // 16 entries (the table is followed by the pad words of the row sort)
    uint32_t *hs = scan + 16;                            // hs[i]: 32-bit hash of the k-mer at position i (hs_cap entries)
    char *sq = reinterpret_cast<char *>(hs + hs_cap);    // the query's bytes
    char *sc = sq + sq_bytes;                            // KF == 31: their complements, 4 pad bytes in front (kmer31_canonical_premix)
    const char *s = one_len ? seqs : seqs + seq_off[q];
    const uint32_t len = one_len ? one_len : (uint32_t)(seq_off[q + 1] - seq_off[q]);
    const uint32_t n = len >= k ? len - k + 1 : 0u;
    const uint64_t P = one_len ? 0ull : pos_off[q];
    uint32_t tsize = 2;
    while (tsize < tab_mult * n) tsize <<= 1;            // load factor <= 1/tab_mult: short probe chains
    const uint32_t mask = tsize - 1;
    for (uint32_t i = threadIdx.x; i < tsize; i += blockDim.x) tab[i] = kEmpty;
    if constexpr (ARGB > 0) {                            // (one_len <= ARGB, zero-padded to a word by the host; sq / sc hold sq_bytes >= that)
        for (uint32_t j = threadIdx.x; j < (len + 3) / 4; j += blockDim.x) {
            const uint32_t w = sarg.w[j];
            reinterpret_cast<uint32_t *>(sq)[j] = w;
            if (KF == 31)
                reinterpret_cast<uint32_t *>(sc + 4)[j] = (uint32_t)complement((uint8_t)w) | (uint32_t)complement((uint8_t)(w >> 8)) << 8 |
                                                          (uint32_t)complement((uint8_t)(w >> 16)) << 16 | (uint32_t)complement((uint8_t)(w >> 24)) << 24;
        }
    } else
    for (uint32_t base = 0; base < len; base += 4 * blockDim.x) {       // four loads in flight per thread and pass
        char c[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t i = base + e * blockDim.x + threadIdx.x;
            c[e] = i < len ? s[i] : (char)0;
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const uint32_t i = base + e * blockDim.x + threadIdx.x;
            if (i >= len) continue;
            sq[i] = c[e];
            if (KF == 31) sc[4 + i] = (char)complement((uint8_t)c[e]);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        if (KF == 31) {
            uint32_t wf[8];
            kmer31_words(reinterpret_cast<const uint32_t *>(sq), i, wf);
            hs[i] = kmer31_fingerprint(wf);
        } else {
            hs[i] = dedupe_hash<KF>(sq + i, k);
        }
    }
    __syncthreads();
    // two positions hold the same k-mer iff their bytes are equal; the stored hashes settle almost every comparison with
    // one LDS word instead of a divergent byte loop
    uint32_t my_slot = 0;                                // where this thread's FIRST position ended up
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t hv = hs[i];
        uint32_t slot = hv & mask;
        for (;;) {
            const uint32_t cur = atomicCAS(&tab[slot], kEmpty, i);
            if (cur == kEmpty) break;
            if (hs[cur] == hv && kmer_equal(sq + cur, sq + i, k)) { atomicMin(&tab[slot], i); break; }
            slot = (slot + 1) & mask;
        }
        if (i == threadIdx.x) my_slot = slot;
    }
    __syncthreads();
    uint32_t *fp = first_pos + P, *ux = uidx + P, *pu = pos_unique + P, *rp = rep_out + P;
    uint64_t *qrows = rows + P * h;
    // (one scan over threads that each take several CONSECUTIVE positions -- fewer barriers -- measured slower: 0.37 against
    // 0.29 ms per 8192 queries; the strided positions keep the LDS reads and the global writes of a wavefront together)
    uint32_t u = 0;
    if (parts > 1) {
        // (n <= blockDim.x: thread i holds position i.)  Ranks as below; then the list of first positions and the rank of every
        // representative go to LDS (the fingerprints and the table are no longer needed), and this part takes its share of both the
        // per-position outputs and the unique k-mers -- whose hashing is repacked onto the first threads of the workgroup.
        const uint32_t i = threadIdx.x;
        const uint32_t c = i < n ? tab[my_slot] : kEmpty;
        const uint32_t flag = (i < n && c == i) ? 1u : 0u;
        const uint32_t pre = block_exclusive_scan_flag(flag != 0, &u, scan);       // (its barrier: every thread has read its table slot)
        if (flag) {
            hs[pre] = i;
            tab[i] = pre;
        }
        __syncthreads();
        const uint32_t pshift = 31u - (uint32_t)__clz((int)parts);         // (parts is a power of two: no division on the chain)
        const uint32_t per_i = (n + parts - 1) >> pshift, i0 = part * per_i, i1 = min(n, i0 + per_i);
        if (i >= i0 && i < i1) {
            rp[i] = c;
            pu[i] = tab[c];
            if (flag) ux[i] = pre;
        }
        const uint32_t per_j = (u + parts - 1) >> pshift, j0 = min(u, part * per_j), j1 = min(u, j0 + per_j);
        for (uint32_t t = threadIdx.x; t < (j1 - j0) * h; t += blockDim.x) {      // a thread per (unique k-mer, seed): the shortest chain
            const uint32_t tj = t / h, j = j0 + tj, sd = t - tj * h, pos = hs[j];
            if (sd == 0) fp[j] = pos;
            kmer_rows<KF>(sq, sc, pos, k, sd, sd + 1, m, qrows + (uint64_t)j * h);
        }
        if (threadIdx.x == 0 && part == 0) {
            num_kmers[q] = n;
            num_unique[q] = u;
            const double mk = ceil((double)u * threshold);
            min_kmers[q] = mk > 0.0 ? (uint32_t)mk : 0u;
        }
        return;
    }
    for (uint32_t base = 0; base < n; base += blockDim.x) {
        const uint32_t i = base + threadIdx.x;
        uint32_t c = kEmpty;
        if (i < n && base == 0) {
            c = tab[my_slot];           // the slot holds the smallest position with this k-mer once all inserts are done
        } else if (i < n) {
            const uint32_t hv = hs[i];
            uint32_t slot = hv & mask;
            for (;;) {
                c = tab[slot];
                if (c == i || (hs[c] == hv && kmer_equal(sq + c, sq + i, k))) break;
                slot = (slot + 1) & mask;
            }
        }
        if (i < n) {
            rp[i] = c;
        }
        const uint32_t flag = (i < n && c == i) ? 1u : 0u;
        uint32_t tot;
        const uint32_t pre = block_exclusive_scan(flag, &tot, scan);
        if (flag) {
            const uint32_t j = u + pre;
            fp[j] = i;
            ux[i] = j;
            kmer_rows<KF>(sq, sc, i, k, 0, h, m, qrows + (uint64_t)j * h);
        }
        u += tot;
    }
    __syncthreads();
    if (rows_sorted) {
        // K1e fused: counting sort of the u*h row ids by their top bits, the dedupe table's LDS reused as the histogram
        // (tsize >= 2n buckets: about one row per bucket at h <= 4).  Order inside a bucket depends on atomics; K2's result does not.
        uint32_t shift = 0;
        while (((m - 1) >> shift) >= (uint64_t)tsize) shift++;
        const uint32_t R = u * h;
        uint64_t *qsorted = rows_sorted + P * h;
        // (phase timestamps: this sort was 23 of a workgroup's 52 us -- two passes of dependent read-backs of the row ids
        // from L2, and 16-way bank conflicts where a thread walks its 16 consecutive buckets.  Now a thread reads its row
        // ids once, all loads in flight together, and keeps them in registers for the second pass; bucket b lives at word
        // b + b / 32, which spreads the threads' bucket runs over the banks.)
        auto at = [](uint32_t b) { return b + (b >> 5); };
        for (uint32_t i = threadIdx.x; i < tsize + (tsize >> 5) + 1; i += blockDim.x) tab[i] = 0;
        __syncthreads();
        constexpr int kSortRegs = 16;
        const bool in_regs = R <= (uint32_t)kSortRegs * blockDim.x;
        uint64_t mine[kSortRegs];
        if (in_regs) {
#pragma unroll
            for (int t = 0; t < kSortRegs; t++) {
                const uint32_t r = threadIdx.x + (uint32_t)t * blockDim.x;
                mine[t] = r < R ? qrows[r] : ~0ull;
            }
#pragma unroll
            for (int t = 0; t < kSortRegs; t++)
                if (mine[t] != ~0ull) atomicAdd(&tab[at((uint32_t)(mine[t] >> shift))], 1u);
        } else {
            for (uint32_t r = threadIdx.x; r < R; r += blockDim.x) atomicAdd(&tab[at((uint32_t)(qrows[r] >> shift))], 1u);
        }
        __syncthreads();
        const uint32_t per = (tsize + blockDim.x - 1) / blockDim.x, b0 = threadIdx.x * per;
        uint32_t sum = 0, tot;
        for (uint32_t j = 0; j < per; j++) sum += b0 + j < tsize ? tab[at(b0 + j)] : 0u;
        uint32_t run = block_exclusive_scan(sum, &tot, scan);
        for (uint32_t j = 0; j < per && b0 + j < tsize; j++) {
            const uint32_t v = tab[at(b0 + j)];
            tab[at(b0 + j)] = run;
            run += v;
        }
        __syncthreads();
        if (in_regs) {
#pragma unroll
            for (int t = 0; t < kSortRegs; t++)
                if (mine[t] != ~0ull) qsorted[atomicAdd(&tab[at((uint32_t)(mine[t] >> shift))], 1u)] = mine[t];
        } else {
            for (uint32_t r = threadIdx.x; r < R; r += blockDim.x) {
                const uint64_t row = qrows[r];
                qsorted[atomicAdd(&tab[at((uint32_t)(row >> shift))], 1u)] = row;
            }
        }
    }
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) pu[i] = ux[rp[i]];
    if (threadIdx.x == 0) {
        num_kmers[q] = n;
        num_unique[q] = u;
        const double mk = ceil((double)u * threshold);
        min_kmers[q] = mk > 0.0 ? (uint32_t)mk : 0u;
    }
}

// K1 for batches whose k-mers arrive as explicit byte strings ("elements", bigsi_hip_batch_create_elements): the host has
// k-merised, deduplicated and canonicalised (a non-ASCII query: the reference windows k CHARACTERS and hashes their UTF-8 bytes,
// utils/fncts.py:38-65, bloom/bloomfilter.py:5-6); what is left of K1 is MurmurHash3 over each element's bytes with seeds
// 0..h-1, the floor-mod, and min_kmers.
__global__ __launch_bounds__(kBlock) void k_rows_raw(
    const char *__restrict__ blob, const uint64_t *__restrict__ elem_off, const uint64_t *__restrict__ seq_elem_off,
    const uint64_t *__restrict__ pos_off, uint32_t h, uint64_t m, double threshold, uint64_t *__restrict__ rows,
    uint32_t *__restrict__ num_kmers, uint32_t *__restrict__ num_unique, uint32_t *__restrict__ min_kmers)
{
    const uint32_t q = blockIdx.x;
    const uint64_t e0 = seq_elem_off[q], P0 = pos_off[q];
    const uint32_t u = (uint32_t)(seq_elem_off[q + 1] - e0);
    for (uint32_t j = threadIdx.x; j < u; j += kBlock) {
        const uint64_t a = elem_off[e0 + j];
        const KmerView v{blob + a, (uint32_t)(elem_off[e0 + j + 1] - a), false};
        for (uint32_t sd = 0; sd < h; sd++) rows[(P0 + j) * h + sd] = row_of_hash(murmur3_32(v, sd), m);
    }
    if (threadIdx.x == 0) {
        num_kmers[q] = (uint32_t)(pos_off[q + 1] - P0);
        num_unique[q] = u;
        const double mk = ceil((double)u * threshold);
        min_kmers[q] = mk > 0.0 ? (uint32_t)mk : 0u;
    }
}

// K1 for probe / read-length queries (at most 64 k-mer positions, e.g. the 61-mers of BASELINE config 2): ONE WAVEFRONT
// PER QUERY, four queries per workgroup, lane i = position i.  Duplicates are found by broadcasting each lane's dedupe
// hash in turn (64 shuffles, string compare only on a hash match), first occurrences are ranked with ballot + popcount:
// no LDS, no atomics, no barriers.  Same outputs as the other two routes.
template <int KF>
__global__ __launch_bounds__(kBlock) void k_kmerize_wave(
    const char *__restrict__ seqs, const uint64_t *__restrict__ seq_off, const uint64_t *__restrict__ pos_off,
    uint32_t k, uint32_t h, uint64_t m, double threshold, uint32_t n_seqs, uint32_t *__restrict__ first_pos,
    uint32_t *__restrict__ pos_unique, uint32_t *__restrict__ rep_out, uint64_t *__restrict__ rows,
    uint32_t *__restrict__ num_kmers, uint32_t *__restrict__ num_unique, uint32_t *__restrict__ min_kmers,
    uint64_t *__restrict__ preset, uint64_t preset_words, uint64_t preset_value, uint64_t *__restrict__ pos_off_out /* as k_kmerize_lds */)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t q = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (q >= n_seqs) return;                       // whole wavefront leaves together
    if (pos_off_out && lane == 0) {
        pos_off_out[q] = pos_off[q];
        if (q + 1 == n_seqs) pos_off_out[n_seqs] = pos_off[n_seqs];
    }
    if (preset) {
        uint64_t *pq = preset + (uint64_t)q * preset_words;
        for (uint64_t i = lane; i < preset_words; i += 64) pq[i] = preset_value;
    }
    const char *s = seqs + seq_off[q];
    const uint32_t len = (uint32_t)(seq_off[q + 1] - seq_off[q]);
    const uint32_t n = len >= k ? len - k + 1 : 0u;      // <= 64 by the launch condition
    const uint64_t P = pos_off[q];
    const bool live = lane < n;
    RegKmer<KF> reg;                               // the k-mer's bytes, loaded once for the fingerprint and the hashes
    uint32_t fp = 0;
    if (KF > 0) {
        if (live) {
            reg.load(s + lane);
            fp = reg.fnv();
        }
    } else if (live) {
        fp = fnv1a(s + lane, k);
    }
    uint32_t rep = lane;
    for (uint32_t j = 0; j + 1 < n; j++) {         // wave-uniform trip count and lane index: a v_readlane, no LDS round trip
        const uint32_t fj = (uint32_t)__builtin_amdgcn_readlane((int)fp, (int)j);
        if (live && lane > j && rep == lane && fp == fj && kmer_equal(s + j, s + lane, k)) rep = j;
    }
    const bool first = live && rep == lane;
    const unsigned long long mask = __ballot(first);
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    const uint32_t u = (uint32_t)__popcll(mask);
    if (live) {
        rep_out[P + lane] = rep;
        pos_unique[P + lane] = (uint32_t)__popcll(mask & (rep ? (~0ull >> (64 - rep)) : 0ull));   // rank of its representative
    }
    if (first) {
        const uint32_t j = (uint32_t)__popcll(mask & below);
        first_pos[P + j] = lane;
        uint64_t *dst = rows + (P + j) * h;
        const char *km = s + lane;
        if (KF > 0) {
            uint32_t w[(KF + 3) / 4 > 0 ? (KF + 3) / 4 : 1];
            reg.canonical_words(w);
            for (uint32_t sd = 0; sd < h; sd++) dst[sd] = row_of_hash(murmur3_words<KF>(w, sd), m);
        } else {
            const KmerView v{km, k, use_revcomp(km, k)};
            for (uint32_t sd = 0; sd < h; sd++) dst[sd] = row_of_hash(murmur3_32(v, sd), m);
        }
    }
    if (lane == 0) {
        num_kmers[q] = n;
        num_unique[q] = u;
        const double mk = ceil((double)u * threshold);
        min_kmers[q] = mk > 0.0 ? (uint32_t)mk : 0u;
    }
}

// ------------------------------------------------------------------------------ K1e: visit rows in address order
// AND (and +1-per-k-mer) are order-free, so each query's row list is bucket-sorted by row id before K2 streams it: all
// resident workgroups then sweep the index from low to high addresses together instead of scattering over 125 GB: with
// launches small enough to be co-resident (bigsi_hip_batch_run) the row-AND kernel runs at 0.857 of peak against 0.79 for
// rows in hash order, whatever the launch size (DRAM page / TLB locality).
// kSortBuckets buckets over [0, m) (about two per row of a 1 kbp query, i.e. nearly a full sort): LDS histogram -> scan -> scatter.  `group` = 1 sorts rows individually (exact path),
// `group` = h keeps each k-mer's h rows together and sorts k-mers by their first row (counting path).
// The order inside a bucket depends on atomics; the results of K2 do not.
constexpr int kSortBuckets = 8192;
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_sort_rows(
    const uint64_t *__restrict__ rows, uint64_t *__restrict__ sorted, const uint64_t *__restrict__ pos_off,
    const uint32_t *__restrict__ num_unique, uint32_t h, uint32_t group, uint32_t shift)
{
    __shared__ uint32_t hist[kSortBuckets];
    __shared__ uint32_t lds[16];
    constexpr int kPer = kSortBuckets / BLOCK;      // consecutive buckets scanned by one thread
    const uint32_t q = blockIdx.x;
    const uint64_t n_items = (uint64_t)num_unique[q] * h / group;
    const uint64_t *src = rows + pos_off[q] * h;
    uint64_t *dst = sorted + pos_off[q] * h;
    for (uint32_t i = threadIdx.x; i < kSortBuckets; i += BLOCK) hist[i] = 0;
    __syncthreads();
    for (uint64_t i = threadIdx.x; i < n_items; i += BLOCK) {
        const uint64_t b = src[i * group] >> shift;
        atomicAdd(&hist[b < kSortBuckets ? b : kSortBuckets - 1], 1u);
    }
    __syncthreads();
    {   // exclusive scan of the histogram
        uint32_t v[kPer], sum = 0;
#pragma unroll
        for (int j = 0; j < kPer; j++) { v[j] = hist[threadIdx.x * kPer + j]; sum += v[j]; }
        uint32_t tot;
        uint32_t run = block_exclusive_scan(sum, &tot, lds);
#pragma unroll
        for (int j = 0; j < kPer; j++) { hist[threadIdx.x * kPer + j] = run; run += v[j]; }
    }
    __syncthreads();
    for (uint64_t i = threadIdx.x; i < n_items; i += BLOCK) {
        const uint64_t b = src[i * group] >> shift;
        const uint32_t pos = atomicAdd(&hist[b < kSortBuckets ? b : kSortBuckets - 1], 1u);
        for (uint32_t s = 0; s < group; s++) dst[(uint64_t)pos * group + s] = src[i * group + s];
    }
}

// ------------------------------------------------------------------------------ K2 work decomposition
// One wavefront streams one 128-word (1 KiB) column segment of every row a query needs: lane l holds words
// [seg*128 + 2l, +2) -> each row read is ONE coalesced 1 KiB wave instruction (global_load_dwordx4), each
// needed byte of a row is read exactly once, and row ids arrive through scalar loads (they are wave-uniform).
// blockIdx -> (query, tile) is XCD-aware: hardware places block b on XCD b % 8, so all tiles of a query get the
// same residue and run on one XCD, adjacent in dispatch order (their row-id lists and the address translations
// of a row's page are shared in that XCD's L2).
// Small batches do not fill the chip that way (one 1 kbp query on a 100k-sample index is 13 wavefronts), so a launch may
// also cut every query's row list into `slices` pieces handled by different workgroups, which combine through atomics
// (AND for the exact bitmap, ADD for counters).  slices == 1 is the plain, atomic-free path used by large batches.
struct TileMap {
    uint32_t q, tile, slice;
    bool valid;
};
// A launch covers the queries [q0, n_seqs): large batches are cut into launches of about a thousand workgroups, all
// co-resident, which then sweep the (address-ordered) row lists together -- a grid several times the chip's residency
// desynchronises that sweep and measured 2.5 % slower at C3.
__device__ __forceinline__ TileMap map_block(uint32_t b, uint32_t q0, uint32_t n_seqs, uint32_t tiles, uint32_t slices = 1)
{
    const uint32_t per_q = tiles * slices;
    if (slices > 1) {
        // a small batch (few queries, sliced): consecutive workgroups -- different XCDs -- take the slices of one query.  With the
        // map below a query lives on ONE XCD, which for a single query is an eighth of the chip and of its bandwidth: one 1 kbp
        // query against 100 k samples took 44 us (1.1 TB/s) at any number of slices.
        const uint32_t ql = b / per_q, rem = b - ql * per_q;
        const uint32_t q = q0 + ql;
        return TileMap{q, rem / slices, rem % slices, q < n_seqs};
    }
    const uint32_t xcd = b & 7u, slot = b >> 3;
    const uint32_t ql = slot / per_q, rem = slot - ql * per_q;
    const uint32_t q = q0 + ql * 8u + xcd;
    return TileMap{q, rem / slices, rem % slices, q < n_seqs};
}

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

template <bool NT = true>
__device__ __forceinline__ u64x2 load_row_seg(const uint64_t *__restrict__ index, uint64_t row, uint64_t stride_words, uint32_t w0)
{
    const u64x2 *p = reinterpret_cast<const u64x2 *>(index + row * stride_words + w0);
    if (NT) return __builtin_nontemporal_load(p);   // streamed once: keep it out of the way of the row-id lists in L2
    return *p;
}

// VEC consecutive 64-column words of a row, streamed: 2 = one 16-byte load (every row kernel's unit), 1 = one 8-byte load
// (k_reads_fused on rows of <= kBlock words: half the registers per lane, twice the lanes that hold columns)
template <int VEC>
struct RowWords;
template <>
struct RowWords<2> {
    u64x2 v;
    static __device__ __forceinline__ RowWords load(const uint64_t *__restrict__ index, uint64_t row, uint64_t stride_words, uint32_t w0) { return RowWords{load_row_seg(index, row, stride_words, w0)}; }
    static __device__ __forceinline__ RowWords fill(uint64_t x) { return RowWords{u64x2{x, x}}; }
    __device__ __forceinline__ RowWords &operator&=(const RowWords &o) { v &= o.v; return *this; }
    __device__ __forceinline__ uint64_t word(int e) const { return e ? v.y : v.x; }
};
template <>
struct RowWords<1> {
    uint64_t v;
    static __device__ __forceinline__ RowWords load(const uint64_t *__restrict__ index, uint64_t row, uint64_t stride_words, uint32_t w0) { return RowWords{__builtin_nontemporal_load(index + row * stride_words + w0)}; }
    static __device__ __forceinline__ RowWords fill(uint64_t x) { return RowWords{x}; }
    __device__ __forceinline__ RowWords &operator&=(const RowWords &o) { v &= o.v; return *this; }
    __device__ __forceinline__ uint64_t word(int) const { return v; }
};

// ------------------------------------------------------------------------------ K2 + K3a: exact
// AND of every row of every unique k-mer of the query (graph/index.py:75-80 then graph/bigsi.py:192-195):
// out[q][w] for w < wv.  Sequences without k-mers produce an all-zero bitmap (the host shim raises for them).
template <int UNROLL, bool NT = true>
__global__ __launch_bounds__(1024) void k_and_exact(
    const uint64_t *__restrict__ index, uint64_t stride_words, uint32_t wv, uint64_t n_cols,
    const uint64_t *__restrict__ rows, const uint64_t *__restrict__ pos_off, const uint32_t *__restrict__ num_unique,
    uint32_t h, uint32_t q0, uint32_t n_seqs, uint32_t tiles, uint64_t *__restrict__ out, uint64_t out_stride_words,
    uint32_t slices /* > 1: `out` was preset to all ones and slices combine with atomicAnd */,
    uint32_t early_exit /* 1: a wavefront stops fetching once its 8192-column segment of the running AND is all zero */)
{
    const TileMap tm = map_block(blockIdx.x, q0, n_seqs, tiles, slices);
    if (!tm.valid) return;
    const uint32_t w0 = (tm.tile * blockDim.x + threadIdx.x) * kVec;
    if (w0 >= wv) return;
    const uint64_t Rall = (uint64_t)num_unique[tm.q] * h;
    const uint64_t per = (Rall + slices - 1) / slices;
    uint64_t r = (uint64_t)tm.slice * per;
    const uint64_t R = r + per < Rall ? r + per : Rall;
    if (slices > 1 && r >= R && Rall != 0) return;        // nothing in this slice
    const uint64_t *qrows = rows + pos_off[tm.q] * h;
    u64x2 acc = {~0ull, ~0ull};
    for (; r + UNROLL <= R; r += UNROLL) {
        u64x2 v[UNROLL];
#pragma unroll
        for (int j = 0; j < UNROLL; j++) v[j] = load_row_seg<NT>(index, qrows[r + j], stride_words, w0);
#pragma unroll
        for (int j = 0; j < UNROLL; j++) acc &= v[j];
        // opt-in (BIGSI_RUN_EARLY_EXIT): no further row can set a bit again, so the result is unchanged; the bytes of the
        // remaining rows are simply not read (NOT used by bench.py, whose algorithmic bytes assume every row is fetched)
        if (early_exit && __ballot((acc.x | acc.y) != 0) == 0) { r = R; break; }
    }
    for (; r < R; r++) acc &= load_row_seg<NT>(index, qrows[r], stride_words, w0);
    if (Rall == 0) acc = u64x2{0ull, 0ull};
    acc.x &= valid_mask(w0, n_cols);
    acc.y &= valid_mask(w0 + 1, n_cols);
    uint64_t *o = out + (uint64_t)tm.q * out_stride_words + w0;
    if (slices > 1) {
        atomicAnd((unsigned long long *)o, (unsigned long long)acc.x);
        if (w0 + 1 < out_stride_words) atomicAnd((unsigned long long *)(o + 1), (unsigned long long)acc.y);
    } else {
        o[0] = acc.x;
        if (w0 + 1 < out_stride_words) o[1] = acc.y;
    }
}

// The same AND as a band sweep (plan_band_sweep, bigsi_launch.hpp): a launch is the 1 KiB column segments [seg0, seg0 + nseg) of EVERY
// query of the batch and the rows [r_lo, r_hi) of their address-ordered lists -- one wavefront per (query, segment), which finds its
// part of the list by binary search (the wavefront's number goes through readfirstlane: the search and the row ids are scalar loads)
// and streams it UNROLL rows at a time.  The first window of a band starts from all ones, a later one from the words the window
// before it left in `out`: each word has one owner and the launches are stream-ordered, so plain load and store are enough.  The last
// window applies valid_mask and the "no k-mers -> all zero" rule.  Plain loads (NT = false) are what lets a row that several queries
// hold be served from cache the second time; non-temporal ones measured no gain from the repeats (profiles/band_sweep_probe.txt).
template <int UNROLL, bool NT>
__global__ __launch_bounds__(kBlock) void k_and_exact_band(
    const uint64_t *__restrict__ index, uint64_t stride_words, uint32_t wv, uint64_t n_cols,
    const uint64_t *__restrict__ rows, const uint64_t *__restrict__ pos_off, const uint32_t *__restrict__ num_unique,
    uint32_t h, uint32_t n_seqs, uint32_t seg0, uint32_t nseg, uint64_t r_lo, uint64_t r_hi, uint32_t first, uint32_t last,
    uint64_t *__restrict__ out, uint64_t out_stride_words)
{
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6))), lane = threadIdx.x & 63u;
    const uint32_t q = wave / nseg;
    if (q >= n_seqs) return;
    const uint32_t w0 = ((seg0 + wave % nseg) * 64u + lane) * kVec;
    if (w0 >= wv) return;
    const uint64_t Rall = (uint64_t)num_unique[q] * h;
    const uint64_t *qrows = rows + pos_off[q] * h;
    uint64_t r = 0, R = Rall;
    for (uint64_t hi = Rall; r < hi;) {          // first row id >= r_lo
        const uint64_t mid = r + ((hi - r) >> 1);
        if (qrows[mid] < r_lo) r = mid + 1;
        else hi = mid;
    }
    for (uint64_t lo = r; lo < R;) {             // first row id >= r_hi
        const uint64_t mid = lo + ((R - lo) >> 1);
        if (qrows[mid] < r_hi) lo = mid + 1;
        else R = mid;
    }
    uint64_t *o = out + (uint64_t)q * out_stride_words + w0;
    const bool two = w0 + 1 < out_stride_words;
    u64x2 acc = {~0ull, ~0ull};
    if (!first) {
        acc.x = o[0];
        if (two) acc.y = o[1];
    }
    for (; r + UNROLL <= R; r += UNROLL) {
        u64x2 v[UNROLL];
#pragma unroll
        for (int j = 0; j < UNROLL; j++) v[j] = load_row_seg<NT>(index, qrows[r + j], stride_words, w0);
#pragma unroll
        for (int j = 0; j < UNROLL; j++) acc &= v[j];
    }
    for (; r < R; r++) acc &= load_row_seg<NT>(index, qrows[r], stride_words, w0);
    if (last) {
        if (Rall == 0) acc = u64x2{0ull, 0ull};
        acc.x &= valid_mask(w0, n_cols);
        acc.y &= valid_mask(w0 + 1, n_cols);
    }
    o[0] = acc.x;
    if (two) o[1] = acc.y;
}

// ------------------------------------------------------------------------------ K2 + K3b: per-sample counts
// For every unique k-mer: AND of its h rows (graph/index.py:75-80), then +1 into the counters of the samples whose
// bit survived (unpack_and_sum, graph/bigsi.py:35-44).  Counters are bit-sliced: P planes of uint64 per word, a
// ripple-carry add of the AND-ed word costs 3 bit-ops per plane, far below what the HBM stream leaves the VALU
// (see DESIGN.md).  Planes are expanded to integers once per (query, segment) and stored as CountT.
template <int P, int H, typename CountT, int KMX = 1 /* 2: software-pipelined loads, for grids too small to fill the SIMDs
    with wavefronts (128 x 4 kbp queries = 2 wavefronts per SIMD: 5.6 -> 6.3 TB/s) */,
          int VEC = kVec /* 64-column words per lane: 2 (16-byte loads), or 1 (8-byte loads: half the plane registers per lane) */>
__global__ __launch_bounds__(kBlock) void k_and_count(
    const uint64_t *__restrict__ index, uint64_t stride_words, uint32_t wv,
    const uint64_t *__restrict__ rows, const uint64_t *__restrict__ pos_off, const uint32_t *__restrict__ num_unique,
    uint32_t h_rt, uint32_t q0, uint32_t n_seqs, uint32_t tiles, CountT *__restrict__ out, uint64_t out_stride /* counters per query */,
    const uint32_t *__restrict__ min_kmers, uint64_t n_cols, uint64_t *__restrict__ hit_bitmap /* [seq][bm_stride] or null */,
    uint64_t bm_stride, uint32_t sparse /* 1: store counters only for words that contain a hit */,
    uint32_t slices /* > 1: a small batch, every query's k-mers cut into slices handled by different workgroups */,
    uint32_t early_exit /* 1 (only with sparse, one slice): a wavefront stops fetching once none of its 8192 columns can reach min_kmers */,
    uint64_t *__restrict__ partial /* slices > 1: where a slice leaves the low `planes_out` planes of its partial counts, bit-sliced as
                                      they are -- [query][slice][plane][bm_stride words]; k_count_combine adds the slices up */,
    uint32_t planes_out)
{
    const TileMap tm = map_block(blockIdx.x, q0, n_seqs, tiles, slices);
    if (!tm.valid) return;
    const uint32_t w0 = (tm.tile * blockDim.x + threadIdx.x) * VEC;
    if (w0 >= wv) return;
    const uint32_t h = H > 0 ? (uint32_t)H : h_rt;
    const uint32_t uall = num_unique[tm.q];
    const uint32_t per = (uall + slices - 1) / slices;
    const uint32_t j0 = tm.slice * per;
    const uint32_t u = j0 + per < uall ? j0 + per : uall;      // this slice covers unique k-mers [j0, u)
    if (slices > 1 && j0 >= u) return;
    const uint64_t *qrows = rows + pos_off[tm.q] * h;
    uint64_t pl[VEC][P];
#pragma unroll
    for (int v = 0; v < VEC; v++)
#pragma unroll
        for (int p = 0; p < P; p++) pl[v][p] = 0;

    auto add = [&](const RowWords<VEC> &a) {
        uint64_t c[VEC];
#pragma unroll
        for (int e = 0; e < VEC; e++) c[e] = a.word(e);
#pragma unroll
        for (int p = 0; p < P; p++) {
#pragma unroll
            for (int e = 0; e < VEC; e++) {          // (the words' carry chains interleaved: independent instructions side by side)
                const uint64_t t = pl[e][p] & c[e];
                pl[e][p] ^= c[e];
                c[e] = t;
            }
        }
    };

    // opt-in (BIGSI_RUN_EARLY_EXIT): with `left` k-mers still to come, a column whose count is below min_kmers - left cannot
    // become a hit any more; when that holds for every column of the wavefront's segment the remaining rows need not be read
    // (same hit lists, fewer bytes than the reference reads -- hence not the default).  One bit-sliced comparison per 32 k-mers.
    const uint32_t thr_exit = early_exit ? min_kmers[tm.q] : 0u;
    auto hopeless = [&](uint32_t left) -> bool {
        if (thr_exit <= left) return false;
        const uint32_t need = thr_exit - left;
        uint64_t any = 0;
#pragma unroll
        for (int v = 0; v < VEC; v++) {
            uint64_t gt = 0, eq = ~0ull;
            if (P < 32 && (need >> (P & 31)) != 0) eq = 0;
#pragma unroll
            for (int p = P - 1; p >= 0; p--) {
                if ((need >> p) & 1u) eq &= pl[v][p];
                else { gt |= eq & pl[v][p]; eq &= ~pl[v][p]; }
            }
            any |= gt | eq;
        }
        return __ballot(any != 0) == 0ull;
    };

    uint32_t j = j0;
    if (H > 0) {
        // KM k-mers per iteration so that 8-12 independent row loads are in flight per lane whatever h is (h=3: 12 loads
        // measured +1.9 % over 6; h=4: 8 vs 16 no difference)
        constexpr int KM0 = H == 1 ? 8 : H <= 3 ? 4 : 2;
        constexpr int KM = KMX == 3 ? (KM0 > 1 ? KM0 / 2 : 1) : KM0;      // KMX == 3: half the loads in flight per lane (launches with > ~1900 live wavefronts)
        if (KMX == 2) {
            // software pipeline: the loads of the NEXT KM k-mers are issued before the bit-sliced adds of the current ones, so
            // a wavefront keeps the memory system busy through its own ALU phase (matters when few wavefronts share a SIMD)
            RowWords<VEC> cur[KM * (H > 0 ? H : 1)], nxt[KM * (H > 0 ? H : 1)];
            if (j + KM <= u) {
#pragma unroll
                for (int s = 0; s < KM * H; s++) cur[s] = RowWords<VEC>::load(index, qrows[(uint64_t)j * H + s], stride_words, w0);
            }
            for (; j + KM <= u; j += KM) {
                const bool more = j + 2 * KM <= u;       // wave-uniform
                if (more) {
#pragma unroll
                    for (int s = 0; s < KM * H; s++) nxt[s] = RowWords<VEC>::load(index, qrows[(uint64_t)(j + KM) * H + s], stride_words, w0);
                }
#pragma unroll
                for (int g = 0; g < KM; g++) {
                    RowWords<VEC> a = cur[g * H];
#pragma unroll
                    for (int s = 1; s < H; s++) a &= cur[g * H + s];
                    add(a);
                }
                if (more) {
#pragma unroll
                    for (int s = 0; s < KM * H; s++) cur[s] = nxt[s];
                }
            }
        } else {
            for (; j + KM <= u; j += KM) {
                if (early_exit && ((j - j0) & 31u) < (uint32_t)KM && j > j0 && hopeless(u - j)) { j = u; break; }
                RowWords<VEC> v[KM * (H > 0 ? H : 1)];
#pragma unroll
                for (int s = 0; s < KM * H; s++) v[s] = RowWords<VEC>::load(index, qrows[(uint64_t)j * H + s], stride_words, w0);
#pragma unroll
                for (int g = 0; g < KM; g++) {
                    RowWords<VEC> a = v[g * H];
#pragma unroll
                    for (int s = 1; s < H; s++) a &= v[g * H + s];
                    add(a);
                }
            }
        }
    }
    for (; j < u; j++) {     // tail k-mers, and every k-mer when h is a run-time value (h > 5): rows in groups of four loads
        const uint64_t *kr = qrows + (uint64_t)j * h;
        RowWords<VEC> a = RowWords<VEC>::fill(~0ull);
        uint32_t s = 0;
        for (; s + 4 <= h; s += 4) {
            RowWords<VEC> l0 = RowWords<VEC>::load(index, kr[s], stride_words, w0), l1 = RowWords<VEC>::load(index, kr[s + 1], stride_words, w0);
            const RowWords<VEC> l2 = RowWords<VEC>::load(index, kr[s + 2], stride_words, w0), l3 = RowWords<VEC>::load(index, kr[s + 3], stride_words, w0);
            l0 &= l2; l1 &= l3; l0 &= l1;
            a &= l0;
        }
        for (; s < h; s++) a &= RowWords<VEC>::load(index, kr[s], stride_words, w0);
        add(a);
    }

    if (slices > 1) {
        // a slice of a small batch: its partial counts stay bit-sliced -- a slice of s k-mers needs ceil(log2(s + 1)) planes, 5 for the
        // 16 k-mers of a 1 kbp query's slice -- and go to scratch memory as coalesced 16-byte stores; k_count_combine adds the slices of
        // a word with bit-sliced adders, thresholds and expands.  (Round 3 expanded every slice's planes to integers and added them
        // with packed atomics: 31 us for one 1 kbp query on 100 k samples, against 14 us for the exact AND of the same rows.)
        uint64_t *o = partial + ((uint64_t)tm.q * slices + tm.slice) * planes_out * bm_stride + w0;
#pragma unroll
        for (int p = 0; p < P; p++)
            if ((uint32_t)p < planes_out) {
                if (VEC == 2) *reinterpret_cast<u64x2 *>(o + (uint64_t)p * bm_stride) = u64x2{pl[0][p], pl[VEC - 1][p]};
                else o[(uint64_t)p * bm_stride] = pl[0][p];
            }
        return;
    }
    // threshold in bit-sliced form (graph/bigsi.py:241-242: count >= min_kmers): MSB-first comparator over the planes,
    // ~2 bit-ops per plane per word; the threshold is wave-uniform so its bit tests are scalar branches
    uint64_t ge[VEC];
    {
        const uint32_t thr = min_kmers[tm.q];
#pragma unroll
        for (int v = 0; v < VEC; v++) {
            uint64_t gt = 0, eq = ~0ull;
            if (P < 32 && (thr >> (P & 31)) != 0) eq = 0;     // threshold above any representable count
#pragma unroll
            for (int p = P - 1; p >= 0; p--) {
                if ((thr >> p) & 1u) eq &= pl[v][p];
                else { gt |= eq & pl[v][p]; eq &= ~pl[v][p]; }
            }
            ge[v] = (gt | eq) & valid_mask((uint64_t)w0 + v, n_cols);
            if (hit_bitmap && (uint64_t)w0 + v < bm_stride) hit_bitmap[(uint64_t)tm.q * bm_stride + w0 + v] = ge[v];
        }
    }

    // expand: column 8b+jj of word w sits at bit 8b+7-jj; 8 consecutive counters per store
#pragma unroll
    for (int v = 0; v < VEC; v++) {
        const uint64_t cbase = ((uint64_t)w0 + v) * 64;
        if (cbase >= out_stride) break;
        if (sparse && ge[v] == 0) continue;
        CountT *o = out + (uint64_t)tm.q * out_stride + cbase;
        // 64 columns x P planes: fully unrolled up to 16 planes; for the 32-plane (> 65535 k-mers) variant the byte loop
        // stays rolled (run-time shift amounts, plane indices still compile-time) to keep the code and registers bounded
        constexpr int kByteUnroll = P > 16 ? 1 : 8;
#pragma unroll kByteUnroll
        for (int b = 0; b < 8; b++) {
            CountT c[8];
#pragma unroll
            for (int jj = 0; jj < 8; jj++) {
                const int bit = 8 * b + 7 - jj;
                uint32_t x = 0;
#pragma unroll
                for (int p = 0; p < P; p++) x |= (uint32_t)((pl[v][p] >> bit) & 1ull) << p;
                c[jj] = (CountT)x;
            }
            if (sizeof(CountT) == 2) {
                uint4 pk;
                pk.x = (uint32_t)c[0] | ((uint32_t)c[1] << 16); pk.y = (uint32_t)c[2] | ((uint32_t)c[3] << 16);
                pk.z = (uint32_t)c[4] | ((uint32_t)c[5] << 16); pk.w = (uint32_t)c[6] | ((uint32_t)c[7] << 16);
                *reinterpret_cast<uint4 *>(o + 8 * b) = pk;
            } else {
                uint4 lo{(uint32_t)c[0], (uint32_t)c[1], (uint32_t)c[2], (uint32_t)c[3]};
                uint4 hi{(uint32_t)c[4], (uint32_t)c[5], (uint32_t)c[6], (uint32_t)c[7]};
                *reinterpret_cast<uint4 *>(o + 8 * b) = lo;
                *reinterpret_cast<uint4 *>(o + 8 * b + 4) = hi;
            }
        }
    }
}


// The slices of a small counting batch added up.  A workgroup owns 32 consecutive 64-column words of one query; its 256 threads are
// 8 groups of 32 (thread = word x group), group g adding the slices g, g + 8, ... of its word with a bit-sliced ripple-carry adder
// (~5 bit-ops per plane), four slices' planes loaded at a time so that a thread has 4 x planes_in loads in flight (one thread per
// word walking all 60 slices of a 1 kbp query was 38 us of dependent round trips).  The eight partial sums meet in LDS; the word is
// thresholded (count >= min_kmers, graph/bigsi.py:241-242) into the hit mask that K4 compacts and column shards exchange, and its
// counters are expanded -- all of them, or (sparse) only those of words that hold a hit -- every group taking one byte (8 columns).
template <int P, typename CountT>
__global__ __launch_bounds__(kBlock) void k_count_combine(
    const uint64_t *__restrict__ partial, uint32_t slices, uint32_t planes_in, uint64_t bm_stride, uint32_t wv, uint32_t n_seqs,
    const uint32_t *__restrict__ num_unique, const uint32_t *__restrict__ min_kmers, uint64_t n_cols, uint64_t *__restrict__ hit_bitmap,
    CountT *__restrict__ out, uint64_t out_stride, uint32_t sparse)
{
    constexpr int G = 8, W = kBlock / G;                 // groups, words per workgroup
    __shared__ uint64_t red[G][P][W];
    const uint32_t wl = threadIdx.x & (W - 1), g = threadIdx.x / W;
    const uint32_t per_q = (wv + W - 1) / W, q = blockIdx.x / per_q, w = (blockIdx.x - q * per_q) * W + wl;
    if (q >= n_seqs) return;                             // (whole workgroup)
    const bool live_w = w < wv;
    // (slices that hold no k-mer of this query wrote nothing: the same rule as k_and_count's early return)
    const uint32_t uall = num_unique[q], per = (uall + slices - 1) / slices;
    const uint32_t live = per ? (uall + per - 1) / per : 0u;
    uint64_t acc[P];
#pragma unroll
    for (int p = 0; p < P; p++) acc[p] = 0;
    const uint64_t slice_words = (uint64_t)planes_in * bm_stride;
    const uint64_t *base = partial + (uint64_t)q * slices * slice_words + w;
    constexpr int KB = 12, PB = 4;
    if (live_w && planes_in <= (uint32_t)PB && live <= (uint32_t)KB * G) {
        // the usual shape of a latency-bound call (<= 96 slices of <= 15 k-mers each: 4 planes): ALL of the group's slices in one
        // batch of loads -- one round trip where the loop below makes three
        uint64_t x[KB][PB];
#pragma unroll
        for (int k = 0; k < KB; k++)
#pragma unroll
            for (int p = 0; p < PB; p++)
                x[k][p] = (g + k * G < live && (uint32_t)p < planes_in) ? base[(uint64_t)(g + k * G) * slice_words + (uint64_t)p * bm_stride] : 0ull;
#pragma unroll
        for (int k = 0; k < KB; k++) {
            uint64_t carry = 0;
#pragma unroll
            for (int p = 0; p < P; p++) {
                const uint64_t a = acc[p];
                if (p < PB) {
                    const uint64_t t = a ^ x[k][p < PB ? p : 0];
                    acc[p] = t ^ carry;
                    carry = (a & x[k][p < PB ? p : 0]) | (carry & t);
                } else {
                    acc[p] = a ^ carry;
                    carry &= a;
                }
            }
        }
    } else if (live_w) {
        for (uint32_t s0 = g; s0 < live; s0 += 4 * G) {
            uint64_t x[4][P];
#pragma unroll
            for (int k = 0; k < 4; k++)
#pragma unroll
                for (int p = 0; p < P; p++)
                    x[k][p] = (s0 + k * G < live && (uint32_t)p < planes_in) ? base[(uint64_t)(s0 + k * G) * slice_words + (uint64_t)p * bm_stride] : 0ull;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                uint64_t carry = 0;
#pragma unroll
                for (int p = 0; p < P; p++) {
                    const uint64_t a = acc[p], t = a ^ x[k][p];
                    acc[p] = t ^ carry;
                    carry = (a & x[k][p]) | (carry & t);
                }
            }
        }
    }
#pragma unroll
    for (int p = 0; p < P; p++) red[g][p][wl] = acc[p];
    __syncthreads();
    if (g == 0) {                                        // the eight partial sums of a word -> its total, into red[0]
#pragma unroll 1
        for (int k = 1; k < G; k++) {
            uint64_t carry = 0;
#pragma unroll
            for (int p = 0; p < P; p++) {
                const uint64_t x = red[k][p][wl], a = acc[p], t = a ^ x;
                acc[p] = t ^ carry;
                carry = (a & x) | (carry & t);
            }
        }
#pragma unroll
        for (int p = 0; p < P; p++) red[0][p][wl] = acc[p];
    }
    __syncthreads();
    if (!live_w) return;
#pragma unroll
    for (int p = 0; p < P; p++) acc[p] = red[0][p][wl];
    const uint32_t thr = min_kmers[q];
    uint64_t gt = 0, eq = ~0ull;
    if (P < 32 && (thr >> (P & 31)) != 0) eq = 0;
#pragma unroll
    for (int p = P - 1; p >= 0; p--) {
        if ((thr >> p) & 1u) eq &= acc[p];
        else { gt |= eq & acc[p]; eq &= ~acc[p]; }
    }
    const uint64_t ge = (gt | eq) & valid_mask(w, n_cols);
    if (g == 0) hit_bitmap[(uint64_t)q * bm_stride + w] = ge;
    if (sparse && ge == 0) return;
    // group g expands byte g of the word: columns 8g .. 8g + 7 (column 8b + jj sits at bit 8b + 7 - jj)
    CountT *o = out + (uint64_t)q * out_stride + (uint64_t)w * 64 + 8 * g;
    CountT c[8];
#pragma unroll
    for (int jj = 0; jj < 8; jj++) {
        const uint32_t bit = 8 * g + 7 - jj;
        uint32_t x = 0;
#pragma unroll
        for (int p = 0; p < P; p++) x |= (uint32_t)((acc[p] >> bit) & 1ull) << p;
        c[jj] = (CountT)x;
    }
    if (sizeof(CountT) == 2) {
        uint4 pk;
        pk.x = (uint32_t)c[0] | ((uint32_t)c[1] << 16); pk.y = (uint32_t)c[2] | ((uint32_t)c[3] << 16);
        pk.z = (uint32_t)c[4] | ((uint32_t)c[5] << 16); pk.w = (uint32_t)c[6] | ((uint32_t)c[7] << 16);
        *reinterpret_cast<uint4 *>(o) = pk;
    } else {
        uint4 lo{(uint32_t)c[0], (uint32_t)c[1], (uint32_t)c[2], (uint32_t)c[3]};
        uint4 hi{(uint32_t)c[4], (uint32_t)c[5], (uint32_t)c[6], (uint32_t)c[7]};
        *reinterpret_cast<uint4 *>(o) = lo;
        *reinterpret_cast<uint4 *>(o + 4) = hi;
    }
}

// ------------------------------------------------------------------------------ K3r: ranked top-N selection (a result limit)
// search(seq, threshold, score, limit=N) == search(seq, threshold, score)[:N]: the reference orders an exact search's hits by
// ascending colour (exact_filter, bigsi/graph/bigsi.py:192-205) and a thresholded one by num_kmers_found, descending, with a STABLE
// sort over ascending colours (inexact_filter, :211-230), then drops deleted samples (:185-190).  So the N results are the hits with
// the highest counts, ties going to the lowest colours, after the excluded (deleted) colours are taken out.  One workgroup per query
// trims the query's hit vector (the AND bitmap, or the count >= min_kmers mask) to those N bits; K4, the export kernels and K5 / K6
// then run unchanged on the trimmed copy (hit lists stay in ascending colour; the host's stable sort restores the reference's order).
//   pass 0     AND-NOT the excluded colours, popcount.  hits <= N: copy the words through, done (one read of the bitmap).
//   select     (counting runs) radix select of the cutoff count c* over v = count - min_kmers, 12-bit digits from the top: an LDS
//              histogram of the digit over the candidates that match the digits chosen so far, a suffix scan over the bins -> the
//              bin that holds the N-th largest, and how many of it still fit.  One pass while num_unique - min_kmers < 4096 (every
//              read, every 1 kbp query), two for gene-length queries, three for the 32-bit counters of > 65 535 k-mers.
//   tie pass   keep count > c*; of the count == c* bits, the first t in colour order: tiles of kBlock consecutive words, the tie
//              counts scanned across the workgroup (block_exclusive_scan) tile by tile.  Exact runs: every hit ties, t = N.
// Counters are read only in words that hold hits (in sparse mode the others are stale), 8 at a time: the 8 columns of one byte of
// the word are 16 B of uint16_t counters (32 B of uint32_t), one vector load.  All loads of the whole-word passes are coalesced
// (thread t takes words t, t + kBlock, ...).  `out` may be `hits` (a group member trims its slot of the gather buffer in place: every
// word is read and written by the same thread in the last pass).
constexpr uint32_t kRankDigitBits = 12, kRankBins = 1u << kRankDigitBits;

// the 8 counters of byte g of word w (columns 64w + 8g .. + 7) as uint32
template <typename CountT>
__device__ __forceinline__ void rank_counts8(const CountT *__restrict__ cq, uint32_t w, uint32_t g, uint32_t c[8])
{
    const CountT *p = cq + (uint64_t)w * 64 + 8 * g;
    if (sizeof(CountT) == 2) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p);
        c[0] = v.x & 0xFFFFu; c[1] = v.x >> 16; c[2] = v.y & 0xFFFFu; c[3] = v.y >> 16;
        c[4] = v.z & 0xFFFFu; c[5] = v.z >> 16; c[6] = v.w & 0xFFFFu; c[7] = v.w >> 16;
    } else {
        const uint4 lo = *reinterpret_cast<const uint4 *>(p), hi = *reinterpret_cast<const uint4 *>(p + 4);
        c[0] = lo.x; c[1] = lo.y; c[2] = lo.z; c[3] = lo.w; c[4] = hi.x; c[5] = hi.y; c[6] = hi.z; c[7] = hi.w;
    }
}

// the lowest n set bits of m
__device__ __forceinline__ uint64_t lowest_bits(uint64_t m, uint32_t n)
{
    if ((uint32_t)__popcll(m) <= n) return m;
    uint64_t r = 0;
    for (uint32_t i = 0; i < n; i++) {
        r |= m & (0ull - m);
        m &= m - 1;
    }
    return r;
}

template <typename CountT>
__global__ __launch_bounds__(kBlock) void k_rank_select(
    const uint64_t *hits, uint64_t stride_words, uint32_t wv, const CountT *__restrict__ counters /* null: exact run */,
    uint64_t counter_stride, const uint32_t *__restrict__ num_unique, const uint32_t *__restrict__ min_kmers,
    const uint64_t *__restrict__ excluded /* null: none; else >= wv words, row format */, uint32_t limit, uint64_t *out)
{
    __shared__ uint32_t hist[kRankBins];
    __shared__ uint32_t lds[16];
    __shared__ uint32_t pick[2];
    const uint32_t q = blockIdx.x;
    const uint64_t *hq = hits + (uint64_t)q * stride_words;
    uint64_t *oq = out + (uint64_t)q * stride_words;
    // pass 0
    uint32_t mine = 0;
    for (uint32_t w = threadIdx.x; w < wv; w += kBlock) {
        uint64_t x = hq[w];
        if (excluded) x &= ~excluded[w];
        mine += (uint32_t)__popcll(x);
    }
    uint32_t total;
    block_exclusive_scan(mine, &total, lds);
    if (total <= limit) {
        if (excluded || oq != hq)
            for (uint32_t w = threadIdx.x; w < wv; w += kBlock) oq[w] = excluded ? hq[w] & ~excluded[w] : hq[w];
        return;
    }
    // radix select of the cutoff (counting runs): prefix / mask = the digits of c* - min_kmers chosen so far
    uint32_t prefix = 0, mask = 0, remaining = limit;
    const uint32_t mk = counters ? min_kmers[q] : 0u;
    const CountT *cq = counters ? counters + (uint64_t)q * counter_stride : nullptr;
    if (counters) {
        const uint32_t range = num_unique[q] > mk ? num_unique[q] - mk : 0u;
        const uint32_t bits = range ? 32u - (uint32_t)__clz(range) : 1u;
        for (int shift = (int)(((bits + kRankDigitBits - 1) / kRankDigitBits - 1) * kRankDigitBits); shift >= 0; shift -= (int)kRankDigitBits) {
            for (uint32_t i = threadIdx.x; i < kRankBins; i += kBlock) hist[i] = 0;
            __syncthreads();
            for (uint32_t w = threadIdx.x; w < wv; w += kBlock) {
                uint64_t x = hq[w];
                if (excluded) x &= ~excluded[w];
                for (uint32_t g = 0; g < 8 && (x >> (8 * g)); g++) {
                    const uint32_t byte = (uint32_t)(x >> (8 * g)) & 0xFFu;
                    if (!byte) continue;
                    uint32_t c[8];
                    rank_counts8(cq, w, g, c);
#pragma unroll
                    for (int jj = 0; jj < 8; jj++) {
                        if (!((byte >> (7 - jj)) & 1u)) continue;      // column 8g + jj sits at bit 8g + 7 - jj
                        const uint32_t v = c[jj] > mk ? c[jj] - mk : 0u;
                        if ((v & mask) == prefix) atomicAdd(&hist[(v >> shift) & (kRankBins - 1)], 1u);
                    }
                }
            }
            __syncthreads();
            // suffix scan: thread t owns bins [16t, 16t + 16); the bin where the running count from the top reaches `remaining`
            constexpr uint32_t per = kRankBins / kBlock;
            uint32_t s = 0;
            for (uint32_t i = 0; i < per; i++) s += hist[threadIdx.x * per + i];
            uint32_t tot;
            const uint32_t pre = block_exclusive_scan(s, &tot, lds);
            uint32_t above = tot - pre - s;
            for (int i = (int)per - 1; i >= 0; i--) {
                const uint32_t bin = threadIdx.x * per + (uint32_t)i, h = hist[bin];
                if (above < remaining && above + h >= remaining) { pick[0] = bin; pick[1] = remaining - above; }
                above += h;
            }
            __syncthreads();
            prefix |= pick[0] << shift;
            mask |= (kRankBins - 1) << shift;
            remaining = pick[1];
            __syncthreads();      // (pick and hist are rewritten by the next digit)
        }
    }
    // tie pass: tiles of kBlock consecutive words, colour order across the workgroup
    uint32_t base = 0;
    for (uint32_t w0 = 0; w0 < wv; w0 += kBlock) {
        const uint32_t w = w0 + threadIdx.x;
        uint64_t x = w < wv ? hq[w] : 0ull;
        if (excluded && w < wv) x &= ~excluded[w];
        uint64_t gt = 0, eq = x;
        if (counters) {
            eq = 0;
            for (uint32_t g = 0; g < 8 && (x >> (8 * g)); g++) {
                const uint32_t byte = (uint32_t)(x >> (8 * g)) & 0xFFu;
                if (!byte) continue;
                uint32_t c[8];
                rank_counts8(cq, w, g, c);
#pragma unroll
                for (int jj = 0; jj < 8; jj++) {
                    if (!((byte >> (7 - jj)) & 1u)) continue;
                    const uint32_t v = c[jj] > mk ? c[jj] - mk : 0u;
                    const uint64_t bit = 1ull << (8 * g + 7 - jj);
                    if (v > prefix) gt |= bit;
                    else if (v == prefix) eq |= bit;
                }
            }
        }
        const uint32_t n_eq = (uint32_t)__popcll(eq);
        uint32_t tot;
        const uint32_t pre = block_exclusive_scan(n_eq, &tot, lds);
        const uint32_t before = base + pre, allow = remaining > before ? min(n_eq, remaining - before) : 0u;
        // the first `allow` ties in COLOUR order: by_column maps the word to column order and back (it is its own inverse)
        const uint64_t kept = allow == n_eq ? eq : allow ? by_column(lowest_bits(by_column(eq), allow)) : 0ull;
        if (w < wv) oq[w] = gt | kept;
        base += tot;
    }
}

// ------------------------------------------------------------------------------ K4: threshold + compaction
// Result buffers are laid out [shard][seq][stride] (n_shards = 1 for a single GPU; > 1 for buffers gathered from column
// shards); hits come out as (colour, count) in (seq, shard, column) order.  The input is always bit vectors (the AND bitmap, or the
// counting kernel's count >= min_kmers mask) and takes two launches (k_hits_totals, k_hits_write).  Colours ascend within a sequence
// (exact_filter's np.where order, graph/bigsi.py:193-204; inexact_filter's dict order before its stable sort, :215-229).
constexpr uint32_t kAllShards = 0xFFFFFFFFu;

// K4 for bit-vector inputs (the AND bitmap of an exact search, the hit mask of a thresholded one) in TWO launches and no
// waiting between workgroups.  Workgroup g owns the `ipb` consecutive items [g * ipb, +ipb) of the (seq, shard, chunk) order;
// the host picks ipb so that the grid is at most kHitsMaxGroups workgroups.
//   k_hits_totals  the group's hit total -> totals[g];
//   k_hits_write   every thread loads a share of the totals of the PRECEDING groups (plain loads: the launch boundary has made
//                  them visible), the workgroup sums them -- the exclusive prefix in one round trip -- and writes its items'
//                  (colour, count) in order (the words come back out of L2).
// Round 2 fused the two into one launch whose workgroups published their totals and spun on those of their predecessors:
// 7 us instead of 14 at BASELINE configs[1], but correct only while every workgroup of the grid was resident -- an assumption
// about the dispatcher and about whatever else runs on the device (other streams, other processes) that nothing enforces.
// The launch boundary costs ~5 us per batch (0.5 % of a 1 ms step at configs[3] / [4]; batches of reads do not come here, they
// write their hits from k_reads_fused) and removes the only unbounded wait the library had.
// (kHitsMaxGroups and the rule that picks ipb: plan_hits, bigsi_launch.hpp)

// item ci of the (seq, shard, chunk) order; the host keeps the number of items below 2^31, so the divisions are 32-bit ones
// (a 64-bit division is a ~100-instruction routine on this hardware: three of them per item were most of K4's time on a
// latency-bound call -- 8.3 us for the seven items of one query on 100 k samples)
struct HitItem {
    uint32_t chunk, shard, q;
};
__device__ __forceinline__ HitItem hit_item(uint64_t ci, uint32_t n_shards, uint32_t chunks)
{
    const uint32_t c32 = (uint32_t)ci, sq = c32 / chunks;
    HitItem it;
    it.chunk = c32 - sq * chunks;
    it.shard = n_shards == 1 ? 0u : sq % n_shards;
    it.q = n_shards == 1 ? sq : sq / n_shards;
    return it;
}

__device__ __forceinline__ uint64_t hits_word(const uint64_t *__restrict__ bitmaps, uint64_t stride_words, uint32_t wv, uint32_t n_seqs,
                                              const HitItem &it, uint32_t *w_out)
{
    const uint32_t w = it.chunk * kBlock + threadIdx.x;   // one 64-column word per thread
    *w_out = w;
    return w < wv ? bitmaps[((uint64_t)it.shard * n_seqs + it.q) * stride_words + w] : 0ull;
}

__global__ __launch_bounds__(kBlock) void k_hits_totals(
    const uint64_t *__restrict__ bitmaps, uint64_t stride_words, uint32_t wv, uint32_t n_seqs, uint32_t n_shards, uint32_t chunks,
    uint32_t ipb, uint32_t *__restrict__ totals)
{
    __shared__ uint32_t lds[16];
    const uint64_t grp = blockIdx.x, n_items = (uint64_t)n_seqs * n_shards * chunks;
    const uint64_t i0 = grp * ipb, i1 = i0 + ipb < n_items ? i0 + ipb : n_items;
    uint32_t mine = 0, w_unused;
    for (uint64_t ci = i0; ci < i1; ci++) mine += (uint32_t)__popcll(hits_word(bitmaps, stride_words, wv, n_seqs, hit_item(ci, n_shards, chunks), &w_unused));
    uint32_t gtot;
    block_exclusive_scan(mine, &gtot, lds);
    if (threadIdx.x == 0) totals[grp] = gtot;
}

__global__ __launch_bounds__(kBlock) void k_hits_write(
    const uint64_t *__restrict__ bitmaps, uint64_t stride_words, uint32_t wv, uint32_t n_seqs, uint32_t n_shards, uint32_t chunks,
    uint64_t shard_cols, const uint32_t *__restrict__ num_unique, uint32_t ipb, const uint32_t *__restrict__ totals,
    uint64_t *__restrict__ hit_off, uint32_t *__restrict__ hit_col, uint32_t *__restrict__ hit_cnt, uint64_t capacity,
    const void *__restrict__ counters, uint32_t counter_bytes, uint64_t counter_stride, uint32_t own_shard,
    uint64_t *exp_out /* non-null (single-workgroup launches of a one-call search only): this launch also writes the caller's block in
                         pinned memory (k_export_results' layout) and raises the flag the host spins on -- no export kernel, one launch
                         boundary less on a call that is a chain of them */,
    uint32_t exp_spec, const uint32_t *__restrict__ exp_uniq, volatile uint64_t *exp_flag, uint64_t exp_serial)
{
    __shared__ uint32_t lds[16];
    __shared__ uint64_t lds64[kBlock / 64];
    if (gridDim.x == 1 && n_shards == 1 && chunks <= 16) {
        // a latency-bound call (one or two gene-length queries, at most 16 items, ONE workgroup): every thread takes a run of
        // CONSECUTIVE words of a query -- all its loads in flight together, one scan per query instead of one per 256 words
        // (7.5 -> ~4 us for one query on 100 k samples)
        uint64_t base = 0;
        // (the block's header numbers: fetched now, beside the words, not in a round trip of their own behind the scans.  What remains of
        // this route's tail is the system-scope release before the flag: 1.5 us by the stamps -- the posted writes' acknowledgement)
        uint32_t hdr = 0;
        const bool hdr_early = 3u * n_seqs <= kBlock;                                 // (a handful of queries: always)
        if (exp_out && hdr_early && threadIdx.x < 3u * n_seqs) hdr = exp_uniq[threadIdx.x];
        for (uint32_t q = 0; q < n_seqs; q++) {
            const uint32_t w_first = threadIdx.x * chunks;
            uint64_t bits[16];
            uint32_t cnt = 0;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const uint32_t w = w_first + j;
                bits[j] = ((uint32_t)j < chunks && w < wv) ? bitmaps[(uint64_t)q * stride_words + w] : 0ull;
                cnt += (uint32_t)__popcll(bits[j]);
            }
            uint32_t tot;
            const uint32_t pre = block_exclusive_scan(cnt, &tot, lds);
            if (threadIdx.x == 0) {
                hit_off[q] = base;
                if (exp_out) exp_out[q] = base;
            }
            uint64_t o = base + pre;
            base += tot;
            if (cnt == 0 || o + cnt > capacity) continue;
            const uint32_t uq = num_unique[q];
            uint32_t *ocol = exp_out ? reinterpret_cast<uint32_t *>(exp_out + n_seqs + 2u) + ((3u * n_seqs + 1u) & ~1u) : nullptr;
#pragma unroll
            for (int j = 0; j < 16; j++) {
                uint64_t mcol = by_column(bits[j]);
                const uint64_t col0 = (uint64_t)(w_first + j) * 64, cnt0 = (uint64_t)q * counter_stride + col0;
                while (mcol) {
                    const uint32_t c = (uint32_t)__builtin_ctzll(mcol);
                    mcol &= mcol - 1;
                    const uint32_t found = !counters ? uq
                                           : counter_bytes == 2 ? (uint32_t) reinterpret_cast<const uint16_t *>(counters)[cnt0 + c]
                                                                : reinterpret_cast<const uint32_t *>(counters)[cnt0 + c];
                    hit_col[o] = (uint32_t)(col0 + c);
                    hit_cnt[o] = found;
                    if (ocol && o < exp_spec) { ocol[o] = (uint32_t)(col0 + c); ocol[exp_spec + o] = found; }
                    o++;
                }
            }
        }
        if (threadIdx.x == 0) hit_off[n_seqs] = base;
        if (exp_out) {
            if (threadIdx.x == 0) { exp_out[n_seqs] = base; exp_out[n_seqs + 1] = 0; }
            uint32_t *o32 = reinterpret_cast<uint32_t *>(exp_out + n_seqs + 2u);
            if (!hdr_early)
                for (uint32_t i = threadIdx.x; i < 3u * n_seqs; i += kBlock) o32[i] = exp_uniq[i];
            else if (threadIdx.x < 3u * n_seqs) o32[threadIdx.x] = hdr;
            __threadfence_system();
            __syncthreads();
            if (threadIdx.x == 0) *exp_flag = exp_serial;
        }
        return;
    }
    const uint64_t grp = blockIdx.x, n_items = (uint64_t)n_seqs * n_shards * chunks;
    const uint64_t i0 = grp * ipb, i1 = i0 + ipb < n_items ? i0 + ipb : n_items;
    // totals of all preceding groups
    uint64_t part = 0;
    for (uint64_t j = threadIdx.x; j < grp; j += kBlock) part += totals[j];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
    if ((threadIdx.x & 63u) == 0) lds64[threadIdx.x >> 6] = part;
    __syncthreads();
    uint64_t base = 0;
#pragma unroll
    for (int i = 0; i < kBlock / 64; i++) base += lds64[i];
    // ordered write (the last group ends up with the grand total in `base`: a grid of ONE group needs no k_hits_totals at all)
    for (uint64_t ci = i0; ci < i1; ci++) {
        uint32_t w;
        const HitItem it = hit_item(ci, n_shards, chunks);
        const uint64_t bits = hits_word(bitmaps, stride_words, wv, n_seqs, it, &w);
        const uint32_t cnt = (uint32_t)__popcll(bits);
        uint32_t tot;
        const uint32_t pre = block_exclusive_scan(cnt, &tot, lds);
        const uint32_t chunk = it.chunk, shard = it.shard, q = it.q;
        if (threadIdx.x == 0 && chunk == 0 && shard == 0) hit_off[q] = base;
        uint64_t o = base + pre;
        base += tot;
        if (cnt == 0 || o + cnt > capacity) continue;     // overflow: the host sees total > capacity, grows the lists, runs this again
        const uint32_t uq = num_unique[q];
        const uint64_t cbase = (uint64_t)shard * shard_cols + (uint64_t)w * 64;
        const bool owned = own_shard == kAllShards || own_shard == shard;
        const uint64_t cnt0 = (own_shard == kAllShards ? (uint64_t)shard * n_seqs + q : (uint64_t)q) * counter_stride + (uint64_t)w * 64;
        for (uint32_t c = 0; c < 64; c++)
            if ((bits >> bit_of_col(c)) & 1ull) {
                hit_col[o] = (uint32_t)(cbase + c);
                hit_cnt[o] = !counters ? uq
                             : !owned ? 0u
                             : counter_bytes == 2 ? (uint32_t) reinterpret_cast<const uint16_t *>(counters)[cnt0 + c]
                                                  : reinterpret_cast<const uint32_t *>(counters)[cnt0 + c];
                o++;
            }
    }
    if (threadIdx.x == 0 && i1 == n_items) hit_off[n_seqs] = base;
}

// ------------------------------------------------------------------------------ reads: K1 + K2 + K4 in ONE launch
// A batch of reads against a narrow index (BASELINE configs[1]: 1000 x 61-mers, 10 000 samples) is three short kernels
// and three launch boundaries: 7 + 24 + 7 us of kernels in a 43 us step.  When every query has < 64 k-mer positions and a row
// fits one workgroup's lanes (<= 512 words), ONE workgroup per query does the whole path: two wavefronts k-merise / dedupe /
// hash (and leave the same arrays in global memory as the K1 kernels, for lookup / presence / fetch_rows), the row ids go to
// the other wavefronts through LDS, all of them stream and AND (or count) the rows, and the workgroup writes its query's hits
// to entries of the hit buffers it allocates with one atomic add (round 4: no order between queries, no waiting; see the
// kernel's last section).  Same results, one launch.
constexpr uint32_t kReadsMaxSeqs = 1u << 20;  // queries per launch of k_reads_fused at most
template <int H, bool EXACT, int VEC = kVec /* 64-column words per lane: 2 (16-byte loads) or 1 (8-byte loads; rows of <= kBlock words) */,
          int UNR_EXACT = 16 /* row loads a lane keeps in flight on the exact route */,
          bool SPLIT = false /* exact route, rows of <= 256 words, a handful of queries (a latency-bound call): the two halves of the
                                workgroup stream half of the query's rows each and meet in LDS -- half the chain of dependent round trips */>
__global__ __launch_bounds__(kBlock) void k_reads_fused(
    const uint64_t *__restrict__ index, uint64_t stride_words, uint32_t wv, uint64_t n_cols, uint64_t m, double threshold,
    const char *__restrict__ seqs, const uint64_t *__restrict__ seq_off, const uint64_t *__restrict__ pos_off, uint32_t n_seqs,
    uint32_t *__restrict__ first_pos, uint32_t *__restrict__ pos_unique, uint32_t *__restrict__ rep_out, uint64_t *__restrict__ rows,
    uint32_t *__restrict__ num_kmers, uint32_t *__restrict__ num_unique, uint32_t *__restrict__ min_kmers,
    uint64_t *__restrict__ out_bits, uint64_t out_stride_words,
    uint64_t *__restrict__ q_start, uint32_t *__restrict__ q_cnt /* per query: where its hits lie in hit_col / hit_cnt, how many */,
    unsigned long long *__restrict__ alloc /* two words: hits allocated so far by this launch [slot] / by the launch before [slot ^ 1] */,
    uint32_t slot, uint32_t *__restrict__ hit_col, uint32_t *__restrict__ hit_cnt,
    uint64_t capacity, uint32_t fp_mask /* ~0; 1 = BIGSI_RUN_WEAK_FINGERPRINT */,
    uint64_t *__restrict__ pos_off_out /* as k_kmerize_lds: inputs come straight from pinned host memory */,
    uint32_t one_len /* as k_kmerize_lds */,
    uint64_t *exp_out /* non-null: a one-call search of ONE read -- the workgroup also writes the caller's block in pinned memory
                         (k_export_reads' layout) and raises the flag the host spins on: no export kernel, no launch boundary */,
    uint32_t exp_spec, volatile uint64_t *exp_flag, uint64_t exp_serial,
    const SeqArg<kSeqArgRead> sarg /* seqs == nullptr (one_len > 0): the one read of the call, passed in the kernel arguments */)
{
    constexpr int KF = 31, P = 6;
    if (pos_off_out && threadIdx.x == 0) {
        if (one_len) {
            pos_off_out[0] = 0;
            pos_off_out[1] = one_len >= (uint32_t)KF ? one_len - KF + 1 : 0u;
        } else {
            pos_off_out[blockIdx.x] = pos_off[blockIdx.x];
            if (blockIdx.x + 1 == n_seqs) pos_off_out[n_seqs] = pos_off[n_seqs];
        }
    }
    __shared__ uint64_t s_rows[64 * H], s_hrow[64 * H];   // row ids: of the unique k-mers / of every position, per seed
    __shared__ uint32_t s_seq[24], s_cmp[25];             // the query's bytes (63 positions + 30 = 93 at most); their complements
    __shared__ uint8_t s_first[64];                       // position of the j-th unique k-mer
    __shared__ uint32_t s_u, s_min;
    __shared__ uint32_t lds[16];
    __shared__ uint64_t lds64[kBlock / 64];
    const uint32_t q = blockIdx.x;
    // ---- K1 on two wavefronts, on packed words.  The query's bytes (<= 93) and their complements are staged in LDS once.
    // Wavefront A finds each k-mer's first occurrence (k_kmerize_wave's scheme with a scalar fast path); wavefront B builds
    // the canonical form of EVERY position (forward words against byte-reversed complement words, compared as big-endian
    // numbers = lexicographically, utils/fncts.py:51-54) and hashes it for all H seeds, sharing the seed-independent part of
    // MurmurHash3.  The rows of the first occurrences are compacted afterwards.  A and B rotate with the query number so that
    // the workgroups sharing a CU load different SIMDs.  (One wavefront working byte by byte was 6.3 us of a 32 us kernel,
    // with the HBM idle: about 4 x 1150 VALU instructions per CU, most of them on one SIMD.)
    {
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        const uint32_t wave_a = (q >> 8) & 3u, wave_b = (wave_a + 2u) & 3u;
        const char *s = one_len ? seqs : seqs + seq_off[q];
        const uint32_t len = one_len ? one_len : (uint32_t)(seq_off[q + 1] - seq_off[q]);
        const uint32_t n = len >= KF ? len - KF + 1 : 0u;      // < 64 by the launch condition
        const uint64_t P0 = one_len ? 0ull : pos_off[q];
        if (threadIdx.x < 100) {                           // s_cmp carries 4 pad bytes in front (the word at byte p - 1 is read)
            const uint32_t t = threadIdx.x;
            uint8_t c = 0;
            if (t < len) c = seqs ? (uint8_t)s[t] : (uint8_t)(sarg.w[t >> 2] >> ((t & 3u) * 8u));
            if (t < 96) {
                reinterpret_cast<uint8_t *>(s_seq)[t] = c;
                reinterpret_cast<uint8_t *>(s_cmp)[4 + t] = complement(c);
            } else {
                reinterpret_cast<uint8_t *>(s_cmp)[t - 96] = 0;
            }
        }
        __syncthreads();
        const bool live = lane < n;
        uint32_t wf[8];                                    // the k-mer at position `lane` (kmer31_words)
        if (wave == wave_a || wave == wave_b) kmer31_words(s_seq, lane, wf);
        if (wave == wave_a) {
            const uint32_t fp = live ? kmer31_fingerprint(wf) & fp_mask : 0u;
            // rep = the first position holding this lane's k-mer.  Branch-free pass: the lowest lane with the same fingerprint
            // (independent v_readlane / compare / select triples, highest lane first so that the lowest match is kept; a serial
            // loop with a scalar early-out ran at 70 ns per position, all dependency stalls), then one word-by-word check
            // against that lane.  A fingerprint collision between different k-mers (2^-32 per pair) sends the wavefront
            // through the exact pairwise loop instead.
            uint32_t cand = lane;
            for (int jb = 48; jb >= 0; jb -= 16) {
                if ((uint32_t)jb >= n) continue;
#pragma unroll
                for (int t = 15; t >= 0; t--) {
                    const uint32_t fj = (uint32_t)__builtin_amdgcn_readlane((int)fp, jb + t);
                    cand = fp == fj ? (uint32_t)(jb + t) : cand;
                }
            }
            cand = min(cand, lane);                        // (lanes at or beyond n are not live and never representatives)
            const bool dup = live && cand < lane;
            bool same = true;
#pragma unroll
            for (int i = 0; i < 8; i++) same = same && (uint32_t)__shfl((int)wf[i], (int)cand, 64) == wf[i];
            uint32_t rep = dup ? cand : lane;
            if (__ballot(dup && !same) != 0ull) {          // wave-uniform, practically never
                rep = lane;
                for (uint32_t j = 0; j + 1 < n; j++) {
                    bool eq = live && lane > j && rep == lane;
#pragma unroll
                    for (int i = 0; i < 8; i++) eq = eq && wf[i] == (uint32_t)__builtin_amdgcn_readlane((int)wf[i], (int)j);
                    if (eq) rep = j;
                }
            }
            const bool first = live && rep == lane;
            const unsigned long long mask = __ballot(first);
            const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
            const uint32_t u = (uint32_t)__popcll(mask);
            if (live) {
                rep_out[P0 + lane] = rep;
                pos_unique[P0 + lane] = (uint32_t)__popcll(mask & (rep ? (~0ull >> (64 - rep)) : 0ull));
            }
            if (first) {
                const uint32_t j = (uint32_t)__popcll(mask & below);
                first_pos[P0 + j] = lane;
                s_first[j] = (uint8_t)lane;
            }
            if (lane == 0) {
                const double mk = ceil((double)u * threshold);
                const uint32_t mn = mk > 0.0 ? (uint32_t)mk : 0u;
                num_kmers[q] = n;
                num_unique[q] = u;
                min_kmers[q] = mn;
                s_u = u;
                s_min = mn;
            }
        }
        if (wave == wave_b) {
            uint32_t k1[8];
            kmer31_canonical_premix(wf, s_cmp, lane, k1);
#pragma unroll
            for (int sd = 0; sd < H; sd++)
                if (live) s_hrow[lane * H + sd] = row_of_hash(murmur3_31_finish(k1, (uint32_t)sd), m);
        }
        __syncthreads();
        if (threadIdx.x < s_u * H) {                      // rows of the unique k-mers, first-occurrence order (u * H <= 252)
            const uint32_t j = threadIdx.x / H, t = threadIdx.x - j * H;
            const uint64_t r = s_hrow[(uint32_t)s_first[j] * H + t];
            s_rows[threadIdx.x] = r;
            rows[P0 * H + threadIdx.x] = r;
        }
    }
    __syncthreads();
    // ---- K2: lane = two words of the row.  (Splitting a query's rows over groups of lanes -- 3 x 79 lanes for the 157-word
    // rows of configs[1] -- so that three times the bytes are in flight measured +-0: with ~1000 workgroups resident the phase
    // already moves 5.7 TB/s of 1.25 KB rows, and the HBM is the limit, not the round trips.)
    const uint32_t u = s_u;
    const uint32_t w0 = (SPLIT ? (threadIdx.x & (kBlock / 2 - 1)) : threadIdx.x) * VEC;
    const bool live = (!SPLIT || threadIdx.x < kBlock / 2) && w0 < wv;      // the lanes that own the query's words from here on
    uint64_t hitw[VEC];
    uint64_t pl[VEC][P];
#pragma unroll
    for (int v = 0; v < VEC; v++) hitw[v] = 0ull;
    if (EXACT) {
        constexpr int UNR = UNR_EXACT;
        const uint32_t R = u * H;
        RowWords<VEC> acc = RowWords<VEC>::fill(~0ull);
        if (SPLIT) {
            __shared__ RowWords<VEC> s_half[kBlock / 2];
            const uint32_t upper = threadIdx.x / (kBlock / 2), Rh = (R + 1) / 2, ra = upper ? Rh : 0u, rb = upper ? R : Rh;
            if (w0 < wv) {
                for (uint32_t r = ra; r < rb; r += UNR) {
                    RowWords<VEC> v[UNR];
#pragma unroll
                    for (int j = 0; j < UNR; j++) v[j] = r + j < rb ? RowWords<VEC>::load(index, s_rows[r + j], stride_words, w0) : RowWords<VEC>::fill(~0ull);
#pragma unroll
                    for (int j = 0; j < UNR; j++) acc &= v[j];
                }
            }
            if (upper) s_half[threadIdx.x - kBlock / 2] = acc;
            __syncthreads();
            if (live) acc &= s_half[threadIdx.x];
        }
        if (live) {
            for (uint32_t r = 0; !SPLIT && r < R; r += UNR) {
                RowWords<VEC> v[UNR];
#pragma unroll
                for (int j = 0; j < UNR; j++) v[j] = r + j < R ? RowWords<VEC>::load(index, s_rows[r + j], stride_words, w0) : RowWords<VEC>::fill(~0ull);
#pragma unroll
                for (int j = 0; j < UNR; j++) acc &= v[j];
            }
            if (R == 0) acc = RowWords<VEC>::fill(0ull);
#pragma unroll
            for (int v = 0; v < VEC; v++) hitw[v] = acc.word(v) & valid_mask((uint64_t)w0 + v, n_cols);
        }
    } else {
#pragma unroll
        for (int v = 0; v < VEC; v++)
#pragma unroll
            for (int p = 0; p < P; p++) pl[v][p] = 0;
        // SPLIT: the upper half of the workgroup counts the k-mers [uh, u), the lower half [0, uh); the partial counts meet in LDS
        const uint32_t upper_c = SPLIT ? threadIdx.x / (kBlock / 2) : 0u, uh = SPLIT ? (u + 1) / 2 : u;
        const uint32_t ja = upper_c ? uh : 0u, jb = SPLIT ? (upper_c ? u : uh) : u;
        if (SPLIT ? w0 < wv : live) {
            constexpr int KM = H <= 2 ? 8 : H == 3 ? 6 : 4;
            for (uint32_t j = ja; j < jb; j += KM) {
                RowWords<VEC> v[KM * H];
#pragma unroll
                for (int t = 0; t < KM * H; t++)
                    v[t] = j + t / H < jb ? RowWords<VEC>::load(index, s_rows[(j + t / H) * H + t % H], stride_words, w0) : RowWords<VEC>::fill(0ull);
#pragma unroll
                for (int g = 0; g < KM; g++) {
                    RowWords<VEC> a = v[g * H];
#pragma unroll
                    for (int t = 1; t < H; t++) a &= v[g * H + t];
#pragma unroll
                    for (int e = 0; e < VEC; e++) {
                        uint64_t c = a.word(e);
#pragma unroll
                        for (int p = 0; p < P; p++) {
                            const uint64_t t0 = pl[e][p] & c;
                            pl[e][p] ^= c;
                            c = t0;
                        }
                    }
                }
            }
        }
        if (SPLIT) {
            __shared__ uint64_t s_pl[P][VEC][kBlock / 2];
            if (upper_c) {
#pragma unroll
                for (int p = 0; p < P; p++)
#pragma unroll
                    for (int e = 0; e < VEC; e++) s_pl[p][e][threadIdx.x - kBlock / 2] = pl[e][p];
            }
            __syncthreads();
            if (live) {          // bit-sliced ripple-carry add of the two partial counts (their sum is at most u < 2^P)
#pragma unroll
                for (int e = 0; e < VEC; e++) {
                    uint64_t carry = 0;
#pragma unroll
                    for (int p = 0; p < P; p++) {
                        const uint64_t a = pl[e][p], b2 = s_pl[p][e][threadIdx.x];
                        pl[e][p] = a ^ b2 ^ carry;
                        carry = (a & b2) | (carry & (a ^ b2));
                    }
                }
            }
        }
        if (live) {
            const uint32_t thr = s_min;
#pragma unroll
            for (int v = 0; v < VEC; v++) {
                uint64_t gt = 0, eq = ~0ull;
                if ((thr >> P) != 0) eq = 0;
#pragma unroll
                for (int p = P - 1; p >= 0; p--) {
                    if ((thr >> p) & 1u) eq &= pl[v][p];
                    else { gt |= eq & pl[v][p]; eq &= ~pl[v][p]; }
                }
                hitw[v] = (gt | eq) & valid_mask((uint64_t)w0 + v, n_cols);
            }
        }
    }
    if (live) {
        uint64_t *o = out_bits + (uint64_t)q * out_stride_words + w0;
#pragma unroll
        for (int v = 0; v < VEC; v++)
            if (w0 + v < out_stride_words) o[v] = hitw[v];
    }
    // ---- K4: this query's hits, at a place of their own.  The workgroup takes `tot` consecutive entries of the batch's hit buffers
    // with ONE atomic add and leaves (start, count) for its query; the lists of different queries lie in whatever order the
    // workgroups got there, and whoever reads them -- the export kernel of the one-call / streaming searches, the host for
    // fetch_hits -- puts them in query order from the counts.  Nobody waits for anybody: rounds 2 and 3 wrote the lists in query
    // order through a publish-and-sum scan whose workgroups spun on the totals of their predecessors (bounded by a timeout and
    // a host-side repeat, but leaning on dispatch order for progress, and 3 us of every 29 us launch).
    uint32_t mine = 0;
#pragma unroll
    for (int v = 0; v < VEC; v++) mine += (uint32_t)__popcll(hitw[v]);
    uint32_t tot;
    const uint32_t pre = block_exclusive_scan(mine, &tot, lds);
    if (threadIdx.x == 0) {
        const uint64_t start = tot ? (uint64_t)atomicAdd(alloc + slot, (unsigned long long)tot) : 0ull;
        lds64[0] = start;
        q_start[q] = start;
        q_cnt[q] = tot;
        if (q == 0) alloc[slot ^ 1u] = 0;          // the next launch of this batch (launches of one batch never overlap) starts from zero
    }
    __syncthreads();
    const uint64_t start = lds64[0];
    if (mine != 0 && start + tot <= capacity) {      // (else the host sees total > capacity, grows the lists and launches again)
        uint64_t o = start + pre;
#pragma unroll
        for (int v = 0; v < VEC; v++) {
            uint64_t mcol = by_column(hitw[v]);
            while (mcol) {
                const uint32_t c = (uint32_t)__builtin_ctzll(mcol);
                mcol &= mcol - 1;
                const uint32_t colour = (uint32_t)(((uint64_t)w0 + v) * 64 + c);
                uint32_t x = u;
                if (!EXACT) {
                    const uint32_t bp = bit_of_col(c);
                    x = 0;
#pragma unroll
                    for (int p = 0; p < P; p++) x |= (uint32_t)((pl[v][p] >> bp) & 1ull) << p;
                }
                hit_col[o] = colour;
                hit_cnt[o] = x;
                if (exp_out && o < exp_spec) {             // (one query: its list starts at 0)
                    uint32_t *ocol = reinterpret_cast<uint32_t *>(exp_out + 3) + 4;      // offsets (2) | 0 | counts (3, padded to 4) | colours | counts
                    ocol[o] = colour;
                    ocol[exp_spec + o] = x;
                }
                o++;
            }
        }
    }
    if (!exp_out) return;
    if (threadIdx.x == 0) {
        exp_out[0] = 0;
        exp_out[1] = tot;
        exp_out[2] = 0;
        uint32_t *o32 = reinterpret_cast<uint32_t *>(exp_out + 3);
        const uint32_t len = one_len ? one_len : (uint32_t)(seq_off[1] - seq_off[0]);
        o32[0] = len >= (uint32_t)KF ? len - KF + 1 : 0u;
        o32[1] = s_u;
        o32[2] = s_min;
    }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) *exp_flag = exp_serial;
}

// ------------------------------------------------------------------------------ lookup (API parity)
// KmerSignatureIndex.lookup for one sequence (graph/index.py:42-49): out[j][w] = AND of the h rows of unique k-mer j.
__global__ __launch_bounds__(kBlock) void k_lookup(
    const uint64_t *__restrict__ index, uint64_t stride_words, uint32_t wv, const uint64_t *__restrict__ qrows,
    uint32_t h, uint32_t u, uint64_t *__restrict__ out)
{
    const uint32_t wblocks = (wv + kBlock - 1) / kBlock;
    const uint32_t j = blockIdx.x / wblocks;
    const uint32_t w = (blockIdx.x % wblocks) * kBlock + threadIdx.x;
    if (j >= u || w >= wv) return;
    uint64_t a = ~0ull;
    for (uint32_t s = 0; s < h; s++) a &= index[qrows[(uint64_t)j * h + s] * stride_words + w];
    out[(uint64_t)j * wv + w] = a;
}

// ------------------------------------------------------------------------------ K5: presence strings
// graph/bigsi.py:232-237: for hit colour c and every k-mer position i (duplicates included), '1' iff every one of the
// k-mer's h rows has bit c set.  out[hit][i] ASCII.
__global__ __launch_bounds__(kBlock) void k_presence(
    const uint64_t *__restrict__ index, uint64_t stride_words, const uint64_t *__restrict__ qrows,
    const uint32_t *__restrict__ pos_unique, uint32_t h, uint32_t n, const uint32_t *__restrict__ colours, uint32_t n_colours,
    uint8_t *__restrict__ out)
{
    const uint32_t pblocks = (n + kBlock - 1) / kBlock;
    const uint32_t hit = blockIdx.x / pblocks;
    const uint32_t i = (blockIdx.x % pblocks) * kBlock + threadIdx.x;
    if (i >= n || hit >= n_colours) return;
    const uint32_t c = colours[hit];
    const uint64_t w = c >> 6, j = pos_unique[i];
    uint64_t a = ~0ull;
    for (uint32_t s = 0; s < h; s++) a &= index[qrows[j * h + s] * stride_words + w];
    out[(uint64_t)hit * n + i] = ((a >> bit_of_col(c & 63u)) & 1ull) ? '1' : '0';
}

// ------------------------------------------------------------------------------ K5 at scale: all hits of a batch in one pass
// BIGSI.score (graph/bigsi.py:232-237) needs, for every hit (sequence q, colour c), the n-character string whose i-th
// character says whether the k-mer at position i is present in sample c.  k_presence above spends h dependent 8-byte loads
// per (hit, position); with thousands of hits per query (threshold 0.4 on a 500k-sample index) that is the wrong unit of
// work.  Here the unit is (unique k-mer, 128-column PAIR OF WORDS that contains hits): the h rows are AND-ed once per pair
// with 16-byte loads, coalesced over the consecutive hit pairs of a query, and ALL hits of the pair take their bit from
// that one AND.  A thread keeps the AND-ed words of 16 unique k-mers in registers and emits, per hit, the 16 presence bits
// as one uint16 (bits[hit][k-mer / 16]); k_presence_expand then writes the ASCII strings over the n positions
// (duplicates included) from those bits.  Bytes: u x h x 16 per hit pair -- the K2 stream restricted to the hit words.
// presence bits of hit number `rank` (rank among the call's hits, each sequence's hits in colour order), unique k-mers
// 16 * chunk .. +15: tiles of 32 ranks, [tile][chunk][rank % 32].  k_presence_bits then stores runs of consecutive ranks
// next to each other (hit-major rows cost it a third of its time in isolated 2-byte stores: 373 vs 251 us without stores,
// 319 us with this layout), and k_presence_expand reads the chunks of 4 consecutive ranks as one 8-byte word.
__device__ __forceinline__ uint64_t presence_bits_at(uint64_t rank, uint32_t chunk, uint32_t n_chunks)
{
    return ((rank >> 5) * n_chunks + chunk) * 32u + (rank & 31u);
}

struct PresencePair {
    uint32_t wpair;          // word pair: columns [128 * wpair, +128)
    uint32_t base;           // rank, among the query's hits sorted by colour, of the pair's first hit (global index into perm)
    uint64_t mask_lo, mask_hi;   // hit bits of the two words (row bit order)
    uint32_t q;              // the query the pair belongs to
    uint32_t reserved;
};
// one wavefront of k_presence_bits: `count` (<= 64) consecutive pairs of ONE query, from pairs[first] on
struct PresenceWave {
    uint32_t first, count;
};


// The grid is flat over wavefronts of pairs (x; a wavefront takes up to 64 pairs of one query: PresenceWave) and 16-k-mer chunks (y): a thresholded search of a few hundred queries of which a
// dozen have hits -- BASELINE configs[4] as benchmarked -- used to launch (pairs of the fullest query / 256) x chunks x queries
// workgroups, nearly all of them empty, and waited for slots beside the next batch's row-AND kernel (166 us against 26 us alone).
template <int H, int WAVES = 2>      // WAVES = 2: the compiler keeps all 16 x h loads of a thread in flight (~200 VGPRs), measured faster than 4
__global__ __launch_bounds__(kBlock, WAVES) void k_presence_bits(
    const uint64_t *__restrict__ index, uint64_t stride_words, const uint64_t *__restrict__ rows, const uint64_t *__restrict__ pos_off,
    const uint32_t *__restrict__ num_unique, uint32_t h_rt, uint32_t n_waves, const PresenceWave *__restrict__ waves,
    const PresencePair *__restrict__ pairs, uint16_t *__restrict__ bits /* presence_bits_at(rank, chunk) */, uint32_t bits_stride)
{
    const uint32_t h = H > 0 ? (uint32_t)H : h_rt;
    const uint32_t jc = blockIdx.y;
    // a wavefront's pairs all belong to one query (the host cuts the pair list that way: round 3 padded every query's pairs to 64
    // entries instead -- 2 KB of upload per query with hits, nearly all of it padding for reads), so the query -- and with it the
    // k-mer count and every row id of the chunk -- is the same for all 64 lanes: scalar loads (per-lane row ids cost this kernel
    // 70 % at 261 k hits)
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)));
    if (w >= n_waves) return;
    const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)waves[w].first);
    const uint32_t count = (uint32_t)__builtin_amdgcn_readfirstlane((int)waves[w].count);
    const uint32_t q = (uint32_t)__builtin_amdgcn_readfirstlane((int)pairs[first].q);
    const uint32_t u = num_unique[q];
    const uint32_t j0 = jc * 16u;
    if (j0 >= u) return;
    if ((threadIdx.x & 63u) >= count) return;
    const PresencePair pr = pairs[first + (threadIdx.x & 63u)];
    const uint64_t *qrows = rows + pos_off[q] * h;
    const uint32_t woff = pr.wpair * 2u;
    const u64x2 zero = {0ull, 0ull};
    u64x2 a[16];
    if (H > 0) {
        // four k-mers = 4 x h independent 16-byte loads in flight, then their ANDs
#pragma unroll
        for (int t0 = 0; t0 < 16; t0 += 4) {
            u64x2 tmp[4 * (H > 0 ? H : 1)];
            constexpr int HH = H > 0 ? H : 1;
#pragma unroll
            for (int x = 0; x < 4 * H; x++) {
                const uint32_t j = j0 + t0 + x / HH;
                tmp[x] = j < u ? load_row_seg(index, qrows[(uint64_t)j * H + x % HH], stride_words, woff) : zero;
            }
#pragma unroll
            for (int t = 0; t < 4; t++) {
                u64x2 v = tmp[t * H];
#pragma unroll
                for (int sidx = 1; sidx < H; sidx++) v &= tmp[t * H + sidx];
                a[t0 + t] = v;
            }
        }
    } else {
#pragma unroll
        for (int t = 0; t < 16; t++) {
            const uint32_t j = j0 + t;
            u64x2 v = zero;
            if (j < u) {
                v = load_row_seg(index, qrows[(uint64_t)j * h], stride_words, woff);
                for (uint32_t sidx = 1; sidx < h; sidx++) v &= load_row_seg(index, qrows[(uint64_t)j * h + sidx], stride_words, woff);
            }
            a[t] = v;
        }
    }
    uint32_t rank = pr.base;
    // (layout: presence_bits_at)
#pragma unroll
    for (int half = 0; half < 2; half++) {
        uint64_t m = by_column(half ? pr.mask_hi : pr.mask_lo);      // bit c set <=> column 64 * word + c is a hit
        while (m) {
            const uint32_t c = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            const uint32_t bp = bit_of_col(c);
            uint32_t out = 0;
#pragma unroll
            for (int t = 0; t < 16; t++) out |= (uint32_t)(((half ? a[t].y : a[t].x) >> bp) & 1ull) << t;
            bits[presence_bits_at(rank, jc, bits_stride)] = (uint16_t)out;
            rank++;
        }
    }
}

// strings: 16 characters per thread, one 16-byte store (every string starts at a multiple of 16 bytes);
// character i of hit t = '0' + bit (unique k-mer of position i) of the hit's presence bits.  Thread -> (hit, 16-character
// piece), `pieces` (a power of two) pieces per hit, flattened over the grid.  A thread needs the position -> unique k-mer map
// of its 16 consecutive positions; read directly that is a 64-byte stride between lanes (one cache line per lane and load:
// measured 0.5 TB/s).  Instead the G = min(pieces, 64) lanes that share a hit fetch its G * 16 entries with 16 coalesced
// loads and pass them through LDS (pitch 20 dwords per lane: conflict-free 16-byte reads).
// Most 16-position pieces of a query hold 16 DISTINCT k-mers that are also new to the query, i.e. consecutive unique indices
// j0 .. j0+15 (always, unless the piece touches a repeat): the piece's characters are then 16 consecutive bits of the hit's
// presence bits.  k_presence_pieces marks those pieces once per call (bit 31 + j0) and lists the others; k_presence_expand
// turns the marked pieces of every hit into characters (two shuffled 16-bit chunks, four 24-bit multiplies: 4 bits -> 4
// bytes), k_presence_expand_listed walks the position -> unique k-mer map for the listed ones.  (The map for every piece ran
// at 1.1 TB/s of string bytes, VALU-bound; keeping it as a fallback inside the fast kernel held that kernel at 4 waves per
// SIMD, latency-bound at 2.6 TB/s.)
__global__ __launch_bounds__(kBlock) void k_presence_pieces(
    const uint32_t *__restrict__ pos_unique, const uint64_t *__restrict__ pos_off, const uint32_t *__restrict__ num_kmers, uint32_t *__restrict__ desc,
    uint32_t *__restrict__ listed_count, uint2 *__restrict__ listed)
{
    const uint32_t q = blockIdx.x, n = num_kmers[q];
    const uint64_t P0 = pos_off[q];
    const uint32_t *pu = pos_unique + P0;
    uint32_t *d = desc + (P0 >> 4) + q;                    // ceil(n / 16) entries per sequence, disjoint by construction
    for (uint32_t pc = threadIdx.x; pc * 16u < n; pc += kBlock) {
        const uint32_t i0 = pc * 16u, cnt = min(16u, n - i0), j0 = pu[i0];
        bool run = true;
        for (uint32_t t = 1; t < cnt; t++) run = run && pu[i0 + t] == j0 + t;
        d[pc] = (j0 & 0x7fffffffu) | (run ? 0x80000000u : 0u);
        if (!run) listed[atomicAdd(listed_count, 1u)] = uint2{q, pc};
    }
}

// the listed pieces (they touch a repeated k-mer): one workgroup per piece at a time, its threads over the hits of the
// piece's sequence; character t of the piece = bit pos_unique[i0 + t] of the hit's presence bits
__global__ __launch_bounds__(kBlock) void k_presence_expand_listed(
    const uint16_t *__restrict__ bits, uint32_t bits_stride, const uint32_t *__restrict__ listed_count, const uint2 *__restrict__ listed,
    const uint64_t *__restrict__ seq_hit_off /* per sequence: its first hit (the hits of a call are grouped by sequence) */,
    const uint64_t *__restrict__ pos_off, const uint32_t *__restrict__ num_kmers, const uint32_t *__restrict__ pos_unique,
    const uint64_t *__restrict__ str_off, uint8_t *__restrict__ out)
{
    const uint32_t count = *listed_count;
    for (uint32_t e = blockIdx.x; e < count; e += gridDim.x) {
        const uint2 ent = listed[e];
        const uint32_t q = ent.x, i0 = ent.y * 16u, n = num_kmers[q], cnt = min(16u, n - i0);
        const uint32_t *pu = pos_unique + pos_off[q] + i0;
        uint32_t j[16];
#pragma unroll
        for (int t = 0; t < 16; t++) j[t] = (uint32_t)t < cnt ? pu[t] : 0u;
        for (uint64_t hit = seq_hit_off[q] + threadIdx.x; hit < seq_hit_off[q + 1]; hit += kBlock) {       // hit = rank
            uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
            for (int t = 0; t < 16; t++) {
                const uint32_t ch = (uint32_t)t < cnt ? '0' + (((uint32_t)bits[presence_bits_at(hit, j[t] >> 4, bits_stride)] >> (j[t] & 15u)) & 1u) : 0u;
                w[t >> 2] |= ch << (8 * (t & 3));
            }
            *reinterpret_cast<uint4 *>(out + str_off[hit] + i0) = uint4{w[0], w[1], w[2], w[3]};
        }
    }
}

// The marked pieces.  A thread writes piece `piece` of kPresenceHits consecutive hits per round, two levels of loads each: the
// hit's record (scalar loads when a whole wavefront shares the hit, ONE_HIT), then the piece's mark and -- independent of it --
// chunk `piece` of the hit's presence bits, one coalesced 2-byte load per lane; the chunk a piece really starts in lies a few
// lanes to the left (unique index <= position) and comes over by a lane shuffle.
constexpr int kPresenceHits = 4, kPresenceRounds = 4;
template <bool ONE_HIT>
__global__ __launch_bounds__(kBlock) void k_presence_expand(
    const uint16_t *__restrict__ bits, uint32_t bits_stride, uint64_t n_hits, uint32_t pieces, const uint32_t *__restrict__ hit_n,
    const uint64_t *__restrict__ hit_pos0 /* per hit: where its sequence's position -> unique map starts */, const uint64_t *__restrict__ str_off,
    uint8_t *__restrict__ out, const uint32_t *__restrict__ hit_seq /* per hit: its sequence */, const uint32_t *__restrict__ desc /* k_presence_pieces */)
    // "hit" = rank throughout: the per-hit arrays arrive in rank order, str_off[rank] is where that hit's string goes
{
    const uint64_t idx = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t shift = 31u - (uint32_t)__builtin_clz(pieces);
    uint32_t group = (uint32_t)(idx >> shift);             // < 2^31 by the launch condition
    if (ONE_HIT) group = (uint32_t)__builtin_amdgcn_readfirstlane((int)group);      // pieces >= 64: the wavefront's lanes share it
    const uint32_t piece = (uint32_t)(idx & (pieces - 1u));
    const uint32_t lane = threadIdx.x & 63u, G = pieces < 64u ? pieces : 64u, sub = lane & (G - 1u);
#pragma unroll 1
    for (uint32_t round = 0; round < (uint32_t)kPresenceRounds; round++) {
        const uint64_t hit0 = ((uint64_t)group * kPresenceRounds + round) * kPresenceHits;
        if (hit0 >= n_hits) break;
        uint32_t n[kPresenceHits], d[kPresenceHits], cw[kPresenceHits];
        uint64_t so[kPresenceHits];
#pragma unroll
        for (int u = 0; u < kPresenceHits; u++) {
            const uint64_t hit = hit0 + u;
            const bool has = hit < n_hits;
            n[u] = has ? hit_n[hit] : 0u;
            so[u] = has ? str_off[hit] : 0ull;
            d[u] = has ? (uint32_t)(hit_pos0[hit] >> 4) + hit_seq[hit] + piece : 0u;       // where the piece's mark is
        }
        {   // chunk `piece` of the four ranks: four neighbouring 16-bit words of one tile (hit0 is a multiple of 4)
            const uint64_t four = *reinterpret_cast<const uint64_t *>(bits + presence_bits_at(hit0, min(piece, bits_stride - 1u), bits_stride));
#pragma unroll
            for (int u = 0; u < kPresenceHits; u++) {
                cw[u] = (uint32_t)(four >> (16 * u)) & 0xffffu;
                d[u] = piece * 16u < n[u] ? desc[d[u]] : 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < kPresenceHits; u++) {
            // a run of consecutive unique k-mers j0 .. : 16 consecutive presence bits, starting in chunk c <= piece
            const uint32_t j0 = d[u] & 0x7fffffffu, c = j0 >> 4, r = j0 & 15u, delta = piece - c;
            uint32_t lo = (uint32_t)__shfl((int)cw[u], (int)(lane - delta), 64);       // (every lane takes part in the shuffles)
            uint32_t hi = (uint32_t)__shfl((int)cw[u], (int)(lane - delta + 1u), 64);
            if (!(d[u] >> 31)) continue;                                             // no piece here, or a listed one
            if (delta > sub) lo = bits[presence_bits_at(hit0 + u, c, bits_stride)];         // the chunk belongs to a lane of another wavefront
            if (r && (delta > sub + 1u || (delta == 0u && sub + 1u >= G))) hi = bits[presence_bits_at(hit0 + u, min(c + 1u, bits_stride - 1u), bits_stride)];
            const uint32_t x16 = (lo | (hi << 16)) >> r, cnt = min(16u, n[u] - piece * 16u);
            uint32_t o[4];
#pragma unroll
            for (int k4 = 0; k4 < 4; k4++) {
                // 4 bits -> 4 bytes: bit i of x lands on bits i, i+7, i+14, i+21 of the product, of which 0, 8, 16, 24 are kept
                const uint32_t x = (x16 >> (4 * k4)) & 15u;
                const uint32_t ch = (__umul24(x, 0x204081u) & 0x01010101u) + 0x30303030u;
                const int valid = (int)cnt - 4 * k4;
                o[k4] = valid >= 4 ? ch : valid <= 0 ? 0u : ch & ((1u << (8 * valid)) - 1u);
            }
            *reinterpret_cast<uint4 *>(out + so[u] + piece * 16u) = uint4{o[0], o[1], o[2], o[3]};
        }
    }
}

// ------------------------------------------------------------------------------ K6: BIGSI.score on the device
// graph/bigsi.py:232-239 + scoring/score.py:7-107.  The reference turns every hit's column of the n x N matrix into a
// '0'/'1' string and scores it in Python.  Here a hit never becomes a string on the device: k_presence_score gathers the
// hit's presence bits into position order -- ONE BIT per k-mer position, in the reference's own bit order
// (bitarray.tobytes() of the presence string), 8x fewer bytes over PCIe than the ASCII strings of k_presence_expand -- and
// runs remove_short_ones / tabulate_score / calculate_score on those bits (bigsi_score.hpp: integer run
// scans + IEEE doubles with Python's round()).  One thread per hit throughout: a hit is ~n / 8 bytes and a few dozen runs,
// and the presence-bit tiles ([tile of 32 ranks][chunk][rank % 32], presence_bits_at) make the threads of a wavefront read
// consecutive 16-bit words.
//
// position-ordered presence bits of every hit AND its score record: thread = rank; piece = 16 positions; marked pieces
// (k_presence_pieces) are 16 consecutive presence bits of the hit, listed ones walk the position -> unique k-mer map (uniform
// over a sequence's hits).  The thread then scores the words it has just written (its own stores: visible to it).
constexpr int kScoreLdsWords = 16;          // presence words of a hit kept in LDS for the scoring passes (16 x 64 = 1024 positions)
__global__ __launch_bounds__(kBlock) void k_presence_score(
    const uint16_t *__restrict__ bits, uint32_t bits_stride, uint64_t n_hits, const uint32_t *__restrict__ hit_n,
    const uint64_t *__restrict__ hit_pos0, const uint32_t *__restrict__ hit_seq, const uint32_t *__restrict__ desc,
    const uint32_t *__restrict__ pos_unique, const uint64_t *__restrict__ out_off /* per rank: byte offset, multiple of 8 */,
    uint8_t *out, const uint32_t *__restrict__ found, const uint32_t *__restrict__ unique, const uint32_t *__restrict__ dest,
    bigsi_score::HitScore *__restrict__ scores)
{
    __shared__ uint64_t lw[kScoreLdsWords][kBlock];       // [word][thread]: conflict-free
    const uint64_t rank = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (rank >= n_hits) return;
    const uint32_t n = hit_n[rank], pieces = (n + 15u) >> 4;
    const uint64_t pos0 = hit_pos0[rank];
    const uint32_t *d = desc + (pos0 >> 4) + hit_seq[rank];
    const uint32_t *pu = pos_unique + pos0;
    const uint16_t *mine = bits + presence_bits_at(rank, 0, bits_stride);      // chunk c of this rank: mine[32 * c]
    uint64_t *dst = reinterpret_cast<uint64_t *>(out + out_off[rank]);
    // four pieces = one 64-position word per round: the four marks, then the (up to) eight 16-bit chunks they point at, as
    // independent loads -- two dependent levels per word instead of two per piece (a thread per hit is a chain of latencies)
    for (uint32_t p0 = 0; p0 < pieces; p0 += 4u) {
        uint32_t mark[4], lo[4], hi[4];
#pragma unroll
        for (int i = 0; i < 4; i++) mark[i] = p0 + i < pieces ? d[p0 + i] : 0x80000000u;      // (beyond the end: "marked", masked to nothing below)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t j0 = mark[i] & 0x7fffffffu, c = j0 >> 4, r = j0 & 15u;
            const bool fast = (mark[i] >> 31) && p0 + i < pieces;
            lo[i] = fast ? (uint32_t)mine[32u * c] : 0u;
            hi[i] = fast && r ? (uint32_t)mine[32u * min(c + 1u, bits_stride - 1u)] : 0u;
        }
        uint64_t acc = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t piece = p0 + i;
            if (piece >= pieces) break;
            const uint32_t cnt = min(16u, n - piece * 16u);
            uint32_t x16;
            if (mark[i] >> 31) {
                x16 = (lo[i] | (hi[i] << 16)) >> (mark[i] & 15u);
            } else {                                    // a piece that touches a repeated k-mer: walk the position -> unique map
                x16 = 0;
                for (uint32_t t = 0; t < cnt; t++) {
                    const uint32_t j = pu[piece * 16u + t];
                    x16 |= (((uint32_t)mine[32u * (j >> 4)] >> (j & 15u)) & 1u) << t;
                }
            }
            x16 &= (1u << cnt) - 1u;
            acc |= (uint64_t)x16 << (16 * i);
        }
        const uint64_t packed = by_column(acc);         // position p -> byte p / 8, mask 0x80 >> (p % 8)
        dst[p0 >> 2] = packed;
        if ((p0 >> 2) < (uint32_t)kScoreLdsWords) lw[p0 >> 2][threadIdx.x] = acc;
    }
    bigsi_score::HitScore rec;
    const uint64_t *w = dst;
    const uint32_t tid = threadIdx.x;
    bigsi_score::score_hit([w, tid](uint32_t k) { return k < (uint32_t)kScoreLdsWords ? lw[k][tid] : by_column(w[k]); }, n, found[rank], unique[rank], &rec);
    scores[dest[rank]] = rec;
}

// scores of every hit from its packed presence bits (row / bitarray order, 8-byte aligned, ceil(n / 64) words each):
// thread = hit; the record of hit t goes to out[dest ? dest[t] : t]
__global__ __launch_bounds__(kBlock) void k_score_packed(
    const uint8_t *__restrict__ packed, const uint64_t *__restrict__ off, uint64_t n_hits, const uint32_t *__restrict__ hit_n,
    const uint32_t *__restrict__ found, const uint32_t *__restrict__ unique, const uint32_t *__restrict__ dest,
    bigsi_score::HitScore *__restrict__ out)
{
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_hits) return;
    const uint64_t *w = reinterpret_cast<const uint64_t *>(packed + off[t]);
    bigsi_score::HitScore rec;
    bigsi_score::score_hit([w](uint32_t k) { return by_column(w[k]); }, hit_n[t], found ? found[t] : 0u, unique ? unique[t] : 0u, &rec);
    out[dest ? dest[t] : t] = rec;
}

// ------------------------------------------------------------------------------ results of a run -> pinned host memory
// What BIGSI.search needs back from a run -- per query: k-mers, unique k-mers, min_kmers, hit offsets; the first `spec` hits --
// written by ONE small kernel straight into a block of pinned host memory the batch owns:
//   [hit_off: n_seqs + 2 uint64 | num_kmers, num_unique, min_kmers: 3 n_seqs uint32 | pad to 8 | colours: spec uint32 | counts: spec uint32]
// instead of three or four device-to-host copies, each with its own ~10 us of latency and a synchronisation: a call then waits
// ONCE, for this kernel's event.  Word n_seqs + 1 of hit_off is the mark of a one-launch read run that gave up (0 otherwise).
// The LAST workgroup to finish then raises a flag word in (coherent) pinned memory, which is what the host spins on: no event
// record, no hipEventSynchronize -- scripts/probe/latency_probe.hip prices the difference.
__global__ __launch_bounds__(kBlock) void k_export_results(
    const uint64_t *__restrict__ hit_off, uint32_t n_seqs, uint32_t with_mark, const uint32_t *__restrict__ uniq,
    const uint32_t *__restrict__ col, const uint32_t *__restrict__ cnt, uint32_t spec, uint64_t *out,
    uint32_t *__restrict__ done_count /* device word, zero between launches */, volatile uint64_t *flag, uint64_t serial)
{
    const uint32_t tid = blockIdx.x * kBlock + threadIdx.x, nt = gridDim.x * kBlock;
    const uint64_t total = hit_off[n_seqs];
    const uint32_t m = (uint32_t)(total < spec ? total : spec);
    for (uint32_t i = tid; i < n_seqs + 2u; i += nt) out[i] = i <= n_seqs ? hit_off[i] : (with_mark ? hit_off[i] : 0ull);
    uint32_t *o32 = reinterpret_cast<uint32_t *>(out + n_seqs + 2u);
    for (uint32_t i = tid; i < 3u * n_seqs; i += nt) o32[i] = uniq[i];
    uint32_t *ocol = o32 + ((3u * n_seqs + 1u) & ~1u), *ocnt = ocol + spec;
    for (uint32_t i = tid; i < m; i += nt) { ocol[i] = col[i]; ocnt[i] = cnt[i]; }
    if (!flag) return;
    __threadfence_system();                     // this thread's stores to host memory are out ...
    __syncthreads();                            // ... and so are the workgroup's
    if (threadIdx.x == 0) {
        if (gridDim.x == 1 || atomicAdd(done_count, 1u) == gridDim.x - 1u) {
            if (gridDim.x > 1) *done_count = 0;
            __threadfence_system();
            *flag = serial;
        }
    }
}

// The same for a one-launch read run, whose hit lists lie in allocation order (k_reads_fused): workgroup g owns a contiguous range
// of queries, sums the hit counts of the queries before its range (plain loads: the launch boundary has published them), scans
// its own, writes the offsets and copies every query's hits to their place in query order.  No workgroup waits for another.
__global__ __launch_bounds__(kBlock) void k_export_reads(
    const uint64_t *__restrict__ q_start, const uint32_t *__restrict__ q_cnt, uint32_t n_seqs, const uint32_t *__restrict__ uniq,
    const uint32_t *__restrict__ col, const uint32_t *__restrict__ cnt, uint64_t capacity /* entries col / cnt hold */, uint32_t spec,
    uint64_t *out, uint32_t *__restrict__ done_count, volatile uint64_t *flag, uint64_t serial)
{
    __shared__ uint32_t lds[16];
    __shared__ uint64_t lds64[kBlock / 64];
    const uint32_t per_g = (n_seqs + gridDim.x - 1) / gridDim.x, q0 = blockIdx.x * per_g < n_seqs ? blockIdx.x * per_g : n_seqs;
    const uint32_t q1 = q0 + per_g < n_seqs ? q0 + per_g : n_seqs;
    uint64_t part = 0;
    for (uint32_t j = threadIdx.x; j < q0; j += kBlock) part += q_cnt[j];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
    if ((threadIdx.x & 63u) == 0) lds64[threadIdx.x >> 6] = part;
    __syncthreads();
    uint64_t base = 0;
#pragma unroll
    for (int i = 0; i < kBlock / 64; i++) base += lds64[i];
    uint32_t *o32 = reinterpret_cast<uint32_t *>(out + n_seqs + 2u);
    uint32_t *ocol = o32 + ((3u * n_seqs + 1u) & ~1u), *ocnt = ocol + spec;
    for (uint32_t qb = q0; qb < q1; qb += kBlock) {
        const uint32_t q = qb + threadIdx.x;
        const uint32_t c = q < q1 ? q_cnt[q] : 0u;
        uint32_t tot;
        const uint32_t pre = block_exclusive_scan(c, &tot, lds);
        const uint64_t off = base + pre;
        base += tot;
        if (q < q1) {
            out[q] = off;
            // (a list the read kernel could not place -- the buffers were full: its start lies beyond them, nothing was written;
            // the total then exceeds the capacity and the host takes the route that grows the buffers)
            const uint64_t src = c ? q_start[q] : 0ull;
            if (src + c <= capacity)
                for (uint32_t j = 0; j < c && off + j < spec; j++) { ocol[off + j] = col[src + j]; ocnt[off + j] = cnt[src + j]; }
        }
    }
    if ((q1 == n_seqs && q0 < n_seqs) || (n_seqs == 0 && blockIdx.x == 0)) {
        if (threadIdx.x == 0) { out[n_seqs] = base; out[n_seqs + 1] = 0; }
    }
    const uint32_t tid = blockIdx.x * kBlock + threadIdx.x, nt = gridDim.x * kBlock;
    for (uint32_t i = tid; i < 3u * n_seqs; i += nt) o32[i] = uniq[i];
    if (!flag) return;
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        if (gridDim.x == 1 || atomicAdd(done_count, 1u) == gridDim.x - 1u) {
            if (gridDim.x > 1) *done_count = 0;
            __threadfence_system();
            *flag = serial;
        }
    }
}

// A one-call search's tables + sequences from the pinned staging to their device arrays: wide coalesced reads over the host link
// (a few hundred requests for 85 KB) in place of the thousands of 64-byte ones k_reads_fused's 1000 workgroups would issue each
// for its own offsets and sequence (measured: 1000 reads of 61 bp in one call 54.8 -> 51.9 us), and of a hipMemcpyAsync whose
// DMA start-up is ~13 us.
__global__ __launch_bounds__(kBlock) void k_stage_in(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint64_t bytes)
{
    const uint64_t n16 = bytes / 16, tid = (uint64_t)blockIdx.x * kBlock + threadIdx.x, nt = (uint64_t)gridDim.x * kBlock;
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
    for (uint64_t i = tid; i < n16; i += nt) d4[i] = s4[i];
    for (uint64_t i = n16 * 16 + tid; i < bytes; i += nt) dst[i] = src[i];
}

// ------------------------------------------------------------------------------ bulk ingest helpers
// n CONSECUTIVE rows [row0, row0 + n) of rb bytes each, packed, to / from the matrix (file <-> HBM: bigsi_hip_load_rows_file /
// save_rows_file when the file's row length is not the device pitch): one workgroup per row, 16-byte lanes where alignment allows.
__global__ __launch_bounds__(kBlock) void k_scatter_run(uint8_t *__restrict__ index, uint64_t stride_bytes, uint64_t row0, const uint8_t *__restrict__ packed, uint64_t rb)
{
    uint8_t *dst = index + (row0 + blockIdx.x) * stride_bytes;
    const uint8_t *src = packed + (uint64_t)blockIdx.x * rb;
    for (uint64_t b = threadIdx.x; b < stride_bytes; b += kBlock) dst[b] = b < rb ? src[b] : (uint8_t)0;
}

__global__ __launch_bounds__(kBlock) void k_gather_run(const uint8_t *__restrict__ index, uint64_t stride_bytes, uint64_t row0, uint8_t *__restrict__ packed, uint64_t rb)
{
    const uint8_t *src = index + (row0 + blockIdx.x) * stride_bytes;
    uint8_t *dst = packed + (uint64_t)blockIdx.x * rb;
    for (uint64_t b = threadIdx.x; b < rb; b += kBlock) dst[b] = b < stride_bytes ? src[b] : (uint8_t)0;
}

// ------------------------------------------------------------------------------ storage contract helpers
// scatter n packed rows (rb bytes each) to rows row_ids[i]; bytes [rb, stride) of the row are zeroed.
__global__ __launch_bounds__(kBlock) void k_scatter_rows(
    uint8_t *__restrict__ index, uint64_t stride_bytes, uint64_t m, const uint64_t *__restrict__ row_ids,
    const uint8_t *__restrict__ packed, uint64_t rb)
{
    const uint64_t i = blockIdx.x;   // one workgroup per row
    const uint64_t row = row_ids[i];
    if (row >= m) return;
    uint8_t *dst = index + row * stride_bytes;
    for (uint64_t b = threadIdx.x; b < stride_bytes; b += kBlock) dst[b] = b < rb ? packed[i * rb + b] : (uint8_t)0;
}

__global__ __launch_bounds__(kBlock) void k_gather_rows(
    const uint8_t *__restrict__ index, uint64_t stride_bytes, uint64_t m, const uint64_t *__restrict__ row_ids,
    uint8_t *__restrict__ packed, uint64_t rb)
{
    const uint64_t i = blockIdx.x;   // one workgroup per row
    const uint64_t row = row_ids[i];
    if (row >= m) return;
    const uint8_t *src = index + row * stride_bytes;
    for (uint64_t b = threadIdx.x; b < rb; b += kBlock) packed[i * rb + b] = b < stride_bytes ? src[b] : (uint8_t)0;
}

// re-stride rows when the column capacity grows (new stride > old stride); runs back to front is not needed because
// the destination is a fresh allocation.
__global__ __launch_bounds__(kBlock) void k_restride(
    const uint64_t *__restrict__ src, uint64_t src_stride, uint64_t *__restrict__ dst, uint64_t dst_stride, uint64_t m)
{
    const uint64_t total = m * dst_stride;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t r = i / dst_stride, w = i - r * dst_stride;
        dst[i] = w < src_stride ? src[r * src_stride + w] : 0ull;
    }
}

// BitMatrix.insert_column / get_column (bigsi/matrix/bitmatrix.py:50-75): bloom bit r <-> bit `col` of row r.
__global__ __launch_bounds__(kBlock) void k_insert_column(
    uint64_t *__restrict__ index, uint64_t stride_words, uint64_t m, uint64_t col, const uint8_t *__restrict__ bloom)
{
    const uint64_t w = col >> 6, bit = bit_of_col((uint32_t)(col & 63u));
    for (uint64_t r = (uint64_t)blockIdx.x * kBlock + threadIdx.x; r < m; r += (uint64_t)gridDim.x * kBlock) {
        const uint64_t on = (bloom[r >> 3] >> (7 - (r & 7))) & 1u;
        uint64_t *p = index + r * stride_words + w;
        *p = (*p & ~(1ull << bit)) | (on << bit);
    }
}

__global__ __launch_bounds__(kBlock) void k_get_column(
    const uint64_t *__restrict__ index, uint64_t stride_words, uint64_t m, uint64_t col, uint8_t *__restrict__ bloom)
{
    // one thread per output byte = 8 rows
    const uint64_t w = col >> 6, bit = bit_of_col((uint32_t)(col & 63u));
    const uint64_t nb = (m + 7) / 8;
    for (uint64_t b = (uint64_t)blockIdx.x * kBlock + threadIdx.x; b < nb; b += (uint64_t)gridDim.x * kBlock) {
        uint32_t v = 0;
        for (uint32_t j = 0; j < 8; j++) {
            const uint64_t r = b * 8 + j;
            if (r < m && ((index[r * stride_words + w] >> bit) & 1ull)) v |= 0x80u >> j;
        }
        bloom[b] = (uint8_t)v;
    }
}

// ------------------------------------------------------------------------------ sample statistics: per-column popcounts
// The vertical popcount of the matrix: for every column the number of rows that have its bit set -- all rows, or (MASKED) the rows a
// Bloom-filter-shaped selector names, which is |A AND B_c| for every sample c at once.  Decomposition as K2 (a wavefront owns one
// 1 KiB column segment, a lane 16 bytes of it; the workgroups of a row block sit side by side over the segments) except that a
// wavefront walks a contiguous block of rows [rb * rows_per_block, +rows_per_block) instead of a row list: the grid is column
// segments x row blocks (plan_col_popcount, bigsi_launch.hpp).  kColPopLoads rows are loaded at a time -- independent 16-byte loads,
// streamed, never reused -- and reduced by a carry-save tree (7 full adders: 8 rows -> one bit each for the planes 1, 2, 4 and a
// carry into plane 8, rippled up the rest), ~7 bit-ops per row and word against k_and_count's 3 per plane.  The kColPopPlanes
// bit-sliced planes hold 2^planes - 1 rows: every flush_groups groups (the host's rule keeps flush_groups * kColPopLoads below that)
// they are expanded -- the row format's permutation, column 8b + jj of a word at bit 8b + 7 - jj -- and added into the wavefront's own
// 32-bit counters, its 8192 entries of partial[row block][column].  Nobody else writes those, so there are no atomics and no
// workgroup waits for another; k_col_popcount_sum adds the row blocks up.  A counter sees at most rows_per_block <= 2^31 rows
// (plan_col_popcount) and the sum is 64 bits wide: nothing wraps for any num_rows.
// MASKED: `mask` is the selector in the row byte format (bit r = byte r / 8 under 0x80 >> (r % 8): what bigsi_hip_get_column and
// bigsi_hip_bloom write), zero-padded to whole 64-row words.  A row block starts at a multiple of 64 rows; its mask words are
// wave-uniform (scalar loads), the wavefront walks their set bits and loads only those rows, 8 at a time; bits at rows >= num_rows are cut off.
template <bool MASKED>
__global__ __launch_bounds__(kBlock) void k_col_popcount(
    const uint64_t *__restrict__ index, uint64_t stride_words, uint64_t num_rows, uint64_t rows_per_block, uint32_t seg_groups,
    uint32_t flush_groups, const uint64_t *__restrict__ mask, uint32_t *__restrict__ partial, uint64_t partial_stride)
{
    constexpr int P = kColPopPlanes, L = kColPopLoads;
    static_assert(L == 8 && P > 3 && P <= 31, "the carry-save tree below takes 8 rows and feeds plane 3");
    const uint64_t rb = blockIdx.x / seg_groups;
    const uint64_t w0 = ((uint64_t)(blockIdx.x - rb * seg_groups) * blockDim.x + threadIdx.x) * kVec;
    if (w0 >= stride_words) return;        // (the stride is a multiple of 16 words: a lane's two words are inside it or both outside)
    const uint64_t r0 = rb * rows_per_block;
    const uint64_t r1 = r0 + rows_per_block < num_rows ? r0 + rows_per_block : num_rows;
    uint32_t *cnt = partial + rb * partial_stride + w0 * 64;

    u64x2 pl[P];
#pragma unroll
    for (int p = 0; p < P; p++) pl[p] = u64x2{0ull, 0ull};
    uint32_t groups = 0;
    bool first = true;

    // full adder on bit vectors: s = a ^ b ^ c, carry = majority(a, b, c)
    auto csa = [](u64x2 &carry, u64x2 &s, u64x2 a, u64x2 b, u64x2 c) {
        const u64x2 u = a ^ b;
        carry = (a & b) | (u & c);
        s = u ^ c;
    };
    auto add8 = [&](const u64x2 (&v)[L]) {
        u64x2 t2a, t2b, t4a, t4b, c8;
        csa(t2a, pl[0], pl[0], v[0], v[1]);
        csa(t2b, pl[0], pl[0], v[2], v[3]);
        csa(t4a, pl[1], pl[1], t2a, t2b);
        csa(t2a, pl[0], pl[0], v[4], v[5]);
        csa(t2b, pl[0], pl[0], v[6], v[7]);
        csa(t4b, pl[1], pl[1], t2a, t2b);
        csa(c8, pl[2], pl[2], t4a, t4b);
#pragma unroll
        for (int p = 3; p < P; p++) {
            const u64x2 t = pl[p] & c8;
            pl[p] ^= c8;
            c8 = t;
        }
    };
    // planes -> this wavefront's counters: 8 consecutive columns (one byte of the row) per pair of 16-byte accesses
    auto flush = [&]() {
#pragma unroll
        for (int e = 0; e < kVec; e++) {
#pragma unroll
            for (int b = 0; b < 8; b++) {
                uint32_t c[8];
#pragma unroll
                for (int jj = 0; jj < 8; jj++) {
                    const int bit = 8 * b + 7 - jj;
                    uint32_t x = 0;
#pragma unroll
                    for (int p = 0; p < P; p++) x |= (uint32_t)(((e ? pl[p].y : pl[p].x) >> bit) & 1ull) << p;
                    c[jj] = x;
                }
                uint4 *o = reinterpret_cast<uint4 *>(cnt + e * 64 + 8 * b);
                uint4 lo{c[0], c[1], c[2], c[3]}, hi{c[4], c[5], c[6], c[7]};
                if (!first) {
                    const uint4 a = o[0], d = o[1];
                    lo.x += a.x; lo.y += a.y; lo.z += a.z; lo.w += a.w;
                    hi.x += d.x; hi.y += d.y; hi.z += d.z; hi.w += d.w;
                }
                o[0] = lo;
                o[1] = hi;
            }
        }
#pragma unroll
        for (int p = 0; p < P; p++) pl[p] = u64x2{0ull, 0ull};
        first = false;
        groups = 0;
    };

    if (MASKED) {
        // wave-uniform walk over the set bits of the block's mask words: a group takes the next 8 selected rows, across word
        // boundaries, so only the block's last group is partly filled
        auto word = [&](uint64_t r) {                      // bit i: row r + i selected
            const uint64_t s = by_column(mask[r >> 6]);
            return r1 - r < 64 ? s & ((1ull << (r1 - r)) - 1) : s;
        };
        uint64_t r = r0, sel = r0 < r1 ? word(r0) : 0;
        for (;;) {
            u64x2 v[L];
            bool any = false;
#pragma unroll
            for (int j = 0; j < L; j++) {
                while (!sel && r + 64 < r1) {
                    r += 64;
                    sel = word(r);
                }
                if (sel) {
                    v[j] = load_row_seg(index, r + (uint64_t)__builtin_ctzll(sel), stride_words, (uint32_t)w0);
                    sel &= sel - 1;
                    any = true;
                } else v[j] = u64x2{0ull, 0ull};
            }
            if (!any) break;
            add8(v);
            if (++groups == flush_groups) flush();
        }
    } else {
        uint64_t r = r0;
        for (; r + L <= r1; r += L) {
            u64x2 v[L];
#pragma unroll
            for (int j = 0; j < L; j++) v[j] = load_row_seg(index, r + j, stride_words, (uint32_t)w0);
            add8(v);
            if (++groups == flush_groups) flush();
        }
        if (r < r1) {
            u64x2 v[L];
#pragma unroll
            for (int j = 0; j < L; j++) v[j] = r + j < r1 ? load_row_seg(index, r + j, stride_words, (uint32_t)w0) : u64x2{0ull, 0ull};
            add8(v);
            groups++;
        }
    }
    if (groups || first) flush();          // (a wavefront without rows still writes its zeros: the sum reads every row block)
}

// out[c] = sum over the row blocks of partial[row block][c], for the columns the index has: the pad columns of the stride are
// never reported, whatever their bits are (bigsi_hip_set_rows can put bits there)
__global__ __launch_bounds__(kBlock) void k_col_popcount_sum(
    const uint32_t *__restrict__ partial, uint64_t partial_stride, uint64_t row_blocks, uint64_t n_cols, uint64_t *__restrict__ out)
{
    const uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= n_cols) return;
    uint64_t s = 0;
#pragma unroll 8
    for (uint64_t b = 0; b < row_blocks; b++) s += partial[b * partial_stride + c];
    out[c] = s;
}

// ------------------------------------------------------------------------------ column compaction: ordered column selection
// Every row becomes the row of its kept columns, in their order, closed up towards column 0; everything from column K to the end of
// the destination stride is zero afterwards.  All that depends on the keep mask alone comes from the host (plan_compact_columns,
// bigsi_launch.hpp): per source word its mask, the six move masks of its compress network and the number of kept columns in front
// of it; per destination word the first source word that feeds it.
// Destination-driven: a wavefront owns kCompactRows whole rows and walks them in ascending chunks of 64 destination words, a lane
// per word.  The lane loops over the source words first_src[o] .. first_src[o + 1] that feed its word: the table entry is loaded
// once for all the rows, the rows' words are kCompactRows independent 8-byte loads, each is compressed (six and / shift / xor / or
// steps; skipped for a mask of all ones, the common word when a few deleted samples are vacuumed), shifted to its bit offset and
// ORed in.  A source word on a boundary is compressed by two lanes.  No atomics, no workgroup waits for another, and the result does
// not depend on the order of execution.  (Tried and measured slower, 95 against 87 ms on 10 M x 100 k at keep density 0.99: every lane
// compressing only its first source word and taking the second from the next lane through a cross-lane shuffle -- the repeated
// loads and bit work of boundary words are not what bounds this kernel.)
// In place (dst == src, same stride) this is correct because compaction only moves bits towards lower columns:
//   - destination word o draws on source words >= o (first_src[o] >= o), so the stores of a chunk [c0, c0 + 64) touch no word that a
//     later chunk reads (those are >= first_src[c0 + 64] >= c0 + 64);
//   - the rows' owner is ONE wavefront: the loop that loads a chunk's sources consumes every load before it ends, for all lanes
//     (they run in lockstep and the wait counter is the wavefront's), and the chunk's stores come after the lanes have left that
//     loop together;
//   - the freed tail [ceil(K / 64), stride) is zeroed after the rows' last chunk.
// Nothing assumes that a row fits anywhere: a chunk is 64 words whatever the width.  (src and dst may alias: no __restrict__.)
__global__ __launch_bounds__(kBlock) void k_compact_columns(
    const uint64_t *src, uint64_t src_stride, uint64_t *dst, uint64_t dst_stride, uint64_t m, const CompactWord *__restrict__ words,
    const uint32_t *__restrict__ first_src, uint64_t dst_words)
{
    constexpr int R = kCompactRows;
    const uint32_t lane = threadIdx.x & 63u, waves_per_block = blockDim.x >> 6;
    const uint64_t wave = (uint64_t)blockIdx.x * waves_per_block + (threadIdx.x >> 6), n_waves = (uint64_t)gridDim.x * waves_per_block;
    for (uint64_t r0 = wave * R; r0 < m; r0 += n_waves * R) {
        const uint32_t nr = m - r0 < (uint64_t)R ? (uint32_t)(m - r0) : (uint32_t)R;      // (wave-uniform)
        const uint64_t *srow[R];
#pragma unroll
        for (int j = 0; j < R; j++) srow[j] = src + (r0 + ((uint32_t)j < nr ? j : 0)) * src_stride;      // (rows past the end: row r0 again, never stored)
        for (uint64_t c0 = 0; c0 < dst_words; c0 += 64) {
            const uint64_t o = c0 + lane;
            uint64_t acc[R];
#pragma unroll
            for (int j = 0; j < R; j++) acc[j] = 0ull;
            if (o < dst_words) {
                const uint64_t s1 = first_src[o + 1];
                const int64_t base = (int64_t)(o * 64);
                for (uint64_t s = first_src[o]; s <= s1; s++) {
                    const uint4 *e = reinterpret_cast<const uint4 *>(words + s);
                    const uint4 e0 = e[0], e3 = e[3];
                    const uint64_t mask = ((uint64_t)e0.y << 32) | e0.x;
                    const int64_t d = (int64_t)e3.z - base;            // bit of this destination word at which the word's kept columns start
                    if (mask == 0ull || d >= 64 || d <= -64) continue;
                    uint64_t v[R];
#pragma unroll
                    for (int j = 0; j < R; j++) v[j] = srow[j][s];
#pragma unroll
                    for (int j = 0; j < R; j++) v[j] = by_column(v[j]);
                    if (mask != ~0ull) {
                        const uint4 e1 = e[1], e2 = e[2];
                        const uint64_t mv[6] = {((uint64_t)e0.w << 32) | e0.z, ((uint64_t)e1.y << 32) | e1.x, ((uint64_t)e1.w << 32) | e1.z,
                                                ((uint64_t)e2.y << 32) | e2.x, ((uint64_t)e2.w << 32) | e2.z, ((uint64_t)e3.y << 32) | e3.x};
#pragma unroll
                        for (int j = 0; j < R; j++) {
                            uint64_t x = v[j] & mask;
#pragma unroll
                            for (int i = 0; i < 6; i++) {
                                const uint64_t t = x & mv[i];
                                x = (x ^ t) | (t >> (1u << i));
                            }
                            v[j] = x;
                        }
                    }
                    // (s >= first_src[o]: the word's last kept column has rank >= 64 o, so d > -64)
#pragma unroll
                    for (int j = 0; j < R; j++) acc[j] |= d >= 0 ? v[j] << d : v[j] >> -d;
                }
            }
            __builtin_amdgcn_wave_barrier();          // the lanes are together again: every load of this chunk has been consumed
            if (o < dst_words) {
#pragma unroll
                for (int j = 0; j < R; j++)
                    if ((uint32_t)j < nr) dst[(r0 + j) * dst_stride + o] = by_column(acc[j]);
            }
        }
        for (uint32_t j = 0; j < nr; j++)
            for (uint64_t w = dst_words + lane; w < dst_stride; w += 64) dst[(r0 + j) * dst_stride + w] = 0ull;
    }
}

// ------------------------------------------------------------------------------ column collapse: OR columns into groups
// Destination column g of every row is the OR of the source columns c with group_of[c] == g; everything from column G to the end of the
// destination stride is zero afterwards.  All that depends on the map alone comes from the host (plan_collapse_columns,
// bigsi_launch.hpp), in terms of bits as they lie in memory: live[w] = the bits of source word w that have a destination, dst_bit[a] =
// the destination bit address of source bit address a.  No by_column here: the row format's permutation is inside the tables.
// Source-driven: a wavefront owns whole rows, one at a time, and an image of the destination row -- or of one WINDOW of it -- in LDS
// (image_words 64-bit words at smem + wavefront-in-workgroup x image_words).  Per row and window:
//   - each lane streams the source row with coalesced 16-byte loads, kCollapseLoads independent ones (and as many of `live`) in flight,
//     ANDs with live, and walks the set bits that are left 32 at a time: b = ctz(x); x &= x - 1.  An all-zero word costs its load;
//   - the dst_bit gathers have L2 latency, so they go in batches: up to kCollapseGathers bit positions are collected, that many loads
//     are issued, then that many LDS ORs (ds_or_b32 without return: bit address a is bit a % 32 of 32-bit word a / 32, in the table, in
//     the source and in the image alike).  A bit whose destination lies outside the window [lo, lo + span) is passed over; the next
//     pass over the row, which then comes from L2, takes it.  Nothing assumes that a destination row fits in LDS;
//   - the image is written out with plain coalesced 16-byte vector stores and cleared for the next window or row.  The last pair may
//     hold one word past ceil(G / 64): nobody ORs into it, it is stored as the zero it is.  The padding words up to the destination
//     stride are stored as zeros without an image behind them.
// ORDER: the image belongs to ONE wavefront, whose LDS instructions execute in program order, and OR is commutative, so the result does
// not depend on the order of execution: no global atomics, no workgroup waits for another, no __syncthreads, no separate zeroing
// launch.  What has to be kept is the COMPILER's order between the ORs of all lanes and the read-out, and between the clear and the
// next ORs: a wavefront-scope fence and a wave barrier at both places (collapse_image_fence).
// Work is proportional to the set bits that move, not to N x G.  All row addressing is 64 bits wide (row x stride passes 2^32 words on
// a 10 M-row index); bit addresses are 32 bits wide (at most 2^32 - 1 columns either side, and the window test wraps correctly).
// Bounds: a source piece p < table_words / 2 and table_words <= src_stride; a destination pair ends at or before
// round_up(ceil(G / 64), 2) <= dst_stride (both strides are multiples of 16 words; the launcher checks the three).
// Loads of the source are plain (several windows read a row again); streamed loads for the one-window case were not tried.
__device__ __forceinline__ void collapse_image_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the set bits of 32 source bits: tab = the dst_bit entries of those 32 bit addresses
__device__ __forceinline__ void collapse_walk(uint32_t x, const uint32_t *__restrict__ tab, uint32_t *img, uint32_t lo, uint32_t span)
{
    constexpr int B = kCollapseGathers;
    while (x) {
        uint32_t d[B];
        bool on[B];
#pragma unroll
        for (int k = 0; k < B; k++) {
            on[k] = x != 0u;
            const uint32_t b = on[k] ? (uint32_t)__builtin_ctz(x) : 0u;
            x &= x - 1u;
            d[k] = on[k] ? tab[b] : 0u;
        }
#pragma unroll
        for (int k = 0; k < B; k++) {
            const uint32_t a = d[k] - lo;          // (wraps for a destination below the window: then a >= span)
            if (on[k] && a < span) atomicOr(&img[a >> 5], 1u << (a & 31u));
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_collapse_columns(
    const uint64_t *__restrict__ src, uint64_t src_stride, uint64_t *__restrict__ dst, uint64_t dst_stride, uint64_t m,
    const uint32_t *__restrict__ dst_bit, const uint64_t *__restrict__ live, uint64_t table_words, uint64_t dst_words, uint64_t window_words,
    uint32_t image_words)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int U = kCollapseLoads;
    const uint32_t lane = threadIdx.x & 63u, wave_in_block = threadIdx.x >> 6, waves_per_block = blockDim.x >> 6;
    const uint64_t wave = (uint64_t)blockIdx.x * waves_per_block + wave_in_block, n_waves = (uint64_t)gridDim.x * waves_per_block;
    uint32_t *img = reinterpret_cast<uint32_t *>(smem) + (size_t)wave_in_block * image_words * 2u;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    for (uint32_t i = lane * 2u; i < image_words; i += 128u) *reinterpret_cast<uint4 *>(img + 2u * i) = zero;
    collapse_image_fence();
    const uint64_t pieces = table_words / 2;          // 16-byte pieces of a source row that carry columns
    const uint4 *live4 = reinterpret_cast<const uint4 *>(live);
    for (uint64_t row = wave; row < m; row += n_waves) {
        const uint4 *srow = reinterpret_cast<const uint4 *>(src + row * src_stride);
        uint64_t *drow = dst + row * dst_stride;
        for (uint64_t win0 = 0; win0 < dst_words; win0 += window_words) {          // (wave-uniform)
            const uint64_t win_n = dst_words - win0 < window_words ? dst_words - win0 : window_words;
            const uint32_t lo = (uint32_t)(win0 * 64), span = (uint32_t)(win_n * 64);
            for (uint64_t p0 = 0; p0 < pieces; p0 += 64 * U) {
                // (a lane past the row's last piece loads that last piece again and walks nothing: a predicated 16-byte load would be
                // split into four 4-byte ones)
                uint4 v[U], lv[U];
                uint64_t p[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint64_t q = p0 + (uint64_t)u * 64 + lane;
                    p[u] = q < pieces ? q : pieces - 1;
                    v[u] = srow[p[u]];
                }
#pragma unroll
                for (int u = 0; u < U; u++) lv[u] = live4[p[u]];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const bool mine = p0 + (uint64_t)u * 64 + lane < pieces;
                    const uint32_t *tab = dst_bit + p[u] * 128;
                    collapse_walk(mine ? v[u].x & lv[u].x : 0u, tab, img, lo, span);
                    collapse_walk(mine ? v[u].y & lv[u].y : 0u, tab + 32, img, lo, span);
                    collapse_walk(mine ? v[u].z & lv[u].z : 0u, tab + 64, img, lo, span);
                    collapse_walk(mine ? v[u].w & lv[u].w : 0u, tab + 96, img, lo, span);
                }
            }
            collapse_image_fence();          // every lane's ORs of this window are in the image
            for (uint64_t i = lane * 2u; i < win_n; i += 128) {
                uint4 *q = reinterpret_cast<uint4 *>(img + 2 * i);
                *reinterpret_cast<uint4 *>(drow + win0 + i) = *q;
                *q = zero;
            }
            collapse_image_fence();          // the image is clear before anybody's next OR
        }
        for (uint64_t w = (dst_words + 1) / 2 * 2 + lane * 2u; w < dst_stride; w += 128) *reinterpret_cast<uint4 *>(drow + w) = zero;
    }
}

// ------------------------------------------------------------------------------ consensus collapse: group columns by member count
// Destination column g of every row is 1 iff at least min_members[g] source columns of group g are set in the row; everything from
// column G to the end of the destination stride is zero afterwards.  k_collapse_columns with COUNTERS in the image: the same
// source-driven walk (a wavefront owns whole rows and its own LDS image of one destination window; 16-byte source loads ANDed with
// live; the set bits walked 32 at a time; table gathers in batches of kCollapseGathers), the tables from plan_consensus_columns
// (bigsi_launch.hpp): dst_col[a] = the destination COLUMN of source bit address a, need[] = the thresholds in read-out order.
//   - a bit whose destination column c lies in the window [lo, lo + span) adds 1 to the field of c: FIELD_BITS bits wide, PER = 32 /
//     FIELD_BITS fields per 32-bit LDS word, field (c - lo) % PER of word (c - lo) / PER (ds_add_u32 without return).  A field never
//     holds more than its group's size and the planner chose FIELD_BITS so that the size fits: no add carries into a neighbour;
//   - read-out, per destination word w of the window: lane l takes the field of column 64 w + (l ^ 7) -- the column whose bit lies
//     at bit l of the word in memory (collapse_mem_bit(l) = l ^ 7 below 64) -- and compares it with need[64 w + l]; the ballot of
//     that predicate IS the memory word: no by_column.  The padding of `need` (kConsensusNever) makes the columns from G on zero, up
//     to the end of the last pair of words, without a bound test.  128 words at a time: lane l keeps the ballots of words 2 l and
//     2 l + 1 and stores them as 16 bytes, so the stores are coalesced like the collapse's;
//   - the part of the image that was used is cleared with 16-byte LDS stores; the stride padding is stored as zeros.
// ORDER: as k_collapse_columns (one wavefront per image, LDS instructions in program order, add is commutative); the compiler's order
// is kept by collapse_image_fence after the adds and after the clear, as there, and once more between the read-out and the clear,
// which here are different lanes' accesses to the same words.  No global atomics, no workgroup waits for another, no __syncthreads.
// 64-bit row addressing; column numbers are 32 bits wide.  Bounds: the collapse's for the source; the read-out loads need[] below
// 64 x round_up(ceil(G / 64), 2) = its size, touches image words below round_up(win_n, 2) x 64 / PER <= image_words x 2 and stores
// pairs that end at or before round_up(ceil(G / 64), 2) <= dst_stride (window_words is even; the launcher checks the rest).
template <int FIELD_BITS>
__device__ __forceinline__ void consensus_walk(uint32_t x, const uint32_t *__restrict__ tab, uint32_t *img, uint32_t lo, uint32_t span)
{
    constexpr int B = kCollapseGathers;
    constexpr uint32_t PER = 32u / FIELD_BITS;
    while (x) {
        uint32_t d[B];
        bool on[B];
#pragma unroll
        for (int k = 0; k < B; k++) {
            on[k] = x != 0u;
            const uint32_t b = on[k] ? (uint32_t)__builtin_ctz(x) : 0u;
            x &= x - 1u;
            d[k] = on[k] ? tab[b] : 0u;
        }
#pragma unroll
        for (int k = 0; k < B; k++) {
            const uint32_t a = d[k] - lo;          // (wraps for a destination below the window: then a >= span)
            if (on[k] && a < span) atomicAdd(&img[a / PER], 1u << ((a % PER) * FIELD_BITS));
        }
    }
}

template <int FIELD_BITS>
__global__ __launch_bounds__(kBlock) void k_consensus_columns(
    const uint64_t *__restrict__ src, uint64_t src_stride, uint64_t *__restrict__ dst, uint64_t dst_stride, uint64_t m,
    const uint32_t *__restrict__ dst_col, const uint64_t *__restrict__ live, const uint32_t *__restrict__ need, uint64_t table_words,
    uint64_t dst_words, uint64_t window_words, uint32_t image_words)
{
    static_assert(FIELD_BITS == 8 || FIELD_BITS == 16 || FIELD_BITS == 32, "fields of 8, 16 or 32 bits");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int U = kCollapseLoads;
    constexpr uint32_t PER = 32u / FIELD_BITS;
    constexpr uint32_t FIELD_MASK = FIELD_BITS == 32 ? 0xFFFFFFFFu : (1u << (FIELD_BITS & 31)) - 1u;
    const uint32_t lane = threadIdx.x & 63u, wave_in_block = threadIdx.x >> 6, waves_per_block = blockDim.x >> 6;
    const uint64_t wave = (uint64_t)blockIdx.x * waves_per_block + wave_in_block, n_waves = (uint64_t)gridDim.x * waves_per_block;
    uint32_t *img = reinterpret_cast<uint32_t *>(smem) + (size_t)wave_in_block * image_words * 2u;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    for (uint32_t i = lane * 4u; i < image_words * 2u; i += 256u) *reinterpret_cast<uint4 *>(img + i) = zero;
    collapse_image_fence();
    const uint64_t pieces = table_words / 2;          // 16-byte pieces of a source row that carry columns
    const uint4 *live4 = reinterpret_cast<const uint4 *>(live);
    const uint32_t my_col = lane ^ 7u;                // the column (within its 64) whose bit is bit `lane` of the word in memory
    for (uint64_t row = wave; row < m; row += n_waves) {
        const uint4 *srow = reinterpret_cast<const uint4 *>(src + row * src_stride);
        uint64_t *drow = dst + row * dst_stride;
        for (uint64_t win0 = 0; win0 < dst_words; win0 += window_words) {          // (wave-uniform)
            const uint64_t win_n = dst_words - win0 < window_words ? dst_words - win0 : window_words;
            const uint32_t lo = (uint32_t)(win0 * 64), span = (uint32_t)(win_n * 64);
            for (uint64_t p0 = 0; p0 < pieces; p0 += 64 * U) {
                // (a lane past the row's last piece loads that last piece again and walks nothing, as in k_collapse_columns)
                uint4 v[U], lv[U];
                uint64_t p[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint64_t q = p0 + (uint64_t)u * 64 + lane;
                    p[u] = q < pieces ? q : pieces - 1;
                    v[u] = srow[p[u]];
                }
#pragma unroll
                for (int u = 0; u < U; u++) lv[u] = live4[p[u]];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const bool mine = p0 + (uint64_t)u * 64 + lane < pieces;
                    const uint32_t *tab = dst_col + p[u] * 128;
                    consensus_walk<FIELD_BITS>(mine ? v[u].x & lv[u].x : 0u, tab, img, lo, span);
                    consensus_walk<FIELD_BITS>(mine ? v[u].y & lv[u].y : 0u, tab + 32, img, lo, span);
                    consensus_walk<FIELD_BITS>(mine ? v[u].z & lv[u].z : 0u, tab + 64, img, lo, span);
                    consensus_walk<FIELD_BITS>(mine ? v[u].w & lv[u].w : 0u, tab + 96, img, lo, span);
                }
            }
            collapse_image_fence();          // every lane's adds of this window are in the image
            const uint32_t pair_n = ((uint32_t)win_n + 1u) & ~1u;          // the words read out: whole pairs (<= 2 x window, 32 bits do)
            const uint32_t *nrow = need + win0 * 64 + lane;
            for (uint32_t b0 = 0; b0 < pair_n; b0 += 128u) {               // (wave-uniform)
                const uint32_t cnt = pair_n - b0 < 128u ? pair_n - b0 : 128u;
                uint64_t w0 = 0ull, w1 = 0ull;
                for (uint32_t i = 0; i < cnt; i++) {          // (not unrolled: the compiler declines to, around the ballot)
                    const uint32_t c = (b0 + i) * 64u + my_col;
                    const uint32_t have = (img[c / PER] >> ((c % PER) * FIELD_BITS)) & FIELD_MASK;
                    const uint64_t word = __ballot(have >= nrow[(uint64_t)(b0 + i) * 64]);
                    if ((i >> 1) == lane) {
                        if (i & 1u) w1 = word;
                        else w0 = word;
                    }
                }
                if (lane * 2u < cnt)
                    *reinterpret_cast<uint4 *>(drow + win0 + b0 + lane * 2u) =
                        make_uint4((uint32_t)w0, (uint32_t)(w0 >> 32), (uint32_t)w1, (uint32_t)(w1 >> 32));
            }
            collapse_image_fence();          // every lane has read its fields before anybody clears them
            for (uint32_t i = lane * 4u; i < pair_n * (2u * FIELD_BITS); i += 256u) *reinterpret_cast<uint4 *>(img + i) = zero;
            collapse_image_fence();          // the image is clear before anybody's next add
        }
        for (uint64_t w = (dst_words + 1) / 2 * 2 + lane * 2u; w < dst_stride; w += 128) *reinterpret_cast<uint4 *>(drow + w) = zero;
    }
}

// ------------------------------------------------------------------------------ row folding: the matrix under a smaller Bloom filter
// dst row r = src row r | src row r + m' | ... | src row r + (factor - 1) m' for r in [0, m'), m' = m_dst: because a row id is
// floor_mod(hash, m) (row_of_hash) and floor_mod(x, m) mod m' == floor_mod(x, m') for every divisor m' of m, this is bit for bit the
// matrix the same samples build under m'.  Decomposition as k_col_popcount: a wavefront owns one 1 KiB column segment, a lane 16 bytes
// of it, and a contiguous block of DESTINATION rows [rb * rows_per_block, +rows_per_block) cut off at m_dst (plan_fold_rows,
// bigsi_launch.hpp); no LDS, no scratch.
//   D > 0: factor == D, known at compile time and < kFoldLoads.  A step folds R = ceil(kFoldLoads / D) destination rows: R x D
//          independent 16-byte loads (8 to 14) are in flight before the first OR.  The rows a block has left over after its whole steps
//          go one at a time (D loads).
//   D == 0: any factor (the launcher sends factors >= kFoldLoads here).  One destination row at a time, its source rows in groups of
//          kFoldLoads independent loads ORed into a running value, the last group predicated (wave-uniform) on the rows that exist.
// The whole destination stride is written: words [0, words) carry columns (the last one masked by tail_mask: bits at columns
// >= num_cols, which bigsi_hip_set_rows can put there, do not survive), words [words, dst_stride) are zero and are not loaded.
// `words` <= src_stride and <= dst_stride; both strides are multiples of kVec words, so a lane's 16 bytes are inside both rows or the
// lane has returned.
// Bounds: a destination row is < r1 <= m_dst; a source row is r + j m' <= (m' - 1) + (factor - 1) m' = m_dst factor - 1.  All row and
// word arithmetic is 64 bits wide: (r + j m') src_stride passes 2^32 words on a 10 M-row index.
// In place (dst == src, equal strides) this is correct without any ordering between lanes:
//   - the rows written are [0, m'); row r is read only as the j = 0 term of itself, by the very lane that writes those 16 bytes, and
//     that lane's store takes its value from that load;
//   - every other source row is >= m' and nobody writes it;
//   - wavefronts own disjoint (segment, row) cells.
// So the result does not depend on the order of execution: no atomics, no barrier, no workgroup waits for another.  (src and dst may
// alias: no __restrict__.)
// Loads are streamed (nontemporal) or plain by kFoldNtLoads.  Streamed is what k_col_popcount does for a matrix that is read once; on
// an MI355X the two flavours were not told apart ("Row folding": their difference is inside the spread between two runs of
// the same build), so the choice is kept as inherited, not as measured faster.  Stores are plain 16-byte vector stores.
constexpr bool kFoldNtLoads = true;
template <bool NT>
__device__ __forceinline__ u64x2 fold_load(const uint64_t *p)
{
    const u64x2 *q = reinterpret_cast<const u64x2 *>(p);
    if (NT) return __builtin_nontemporal_load(q);
    return *q;
}

template <int D, bool NT>
__global__ __launch_bounds__(kBlock) void k_fold_rows(
    const uint64_t *src, uint64_t src_stride, uint64_t *dst, uint64_t dst_stride, uint64_t m_dst, uint64_t factor, uint64_t words,
    uint64_t tail_mask, uint64_t rows_per_block, uint32_t seg_groups)
{
    constexpr int L = kFoldLoads, R = D > 0 ? (L + D - 1) / D : 1;
    static_assert(D >= 0 && D < L && R * (D > 0 ? D : L) <= kFoldMaxLoads, "plan_fold_rows' invariant: at most kFoldMaxLoads loads per lane and step");
    const uint64_t rb = blockIdx.x / seg_groups;
    const uint64_t w0 = ((uint64_t)(blockIdx.x - rb * seg_groups) * blockDim.x + threadIdx.x) * kVec;
    if (w0 >= dst_stride) return;
    const uint64_t r0 = rb * rows_per_block;
    if (r0 >= m_dst) return;
    const uint64_t r1 = m_dst - r0 > rows_per_block ? r0 + rows_per_block : m_dst;
    uint64_t *out = dst + r0 * dst_stride + w0;
    if (w0 >= words) {          // the pad of the destination stride: zero, nothing to read
        for (uint64_t r = r0; r < r1; r++, out += dst_stride) *reinterpret_cast<u64x2 *>(out) = u64x2{0ull, 0ull};
        return;
    }
    const u64x2 keep{w0 + 1 < words ? ~0ull : tail_mask, w0 + 2 < words ? ~0ull : (w0 + 2 == words ? tail_mask : 0ull)};
    const uint64_t fold = m_dst * src_stride;          // words between two terms of a destination row
    const uint64_t *in = src + r0 * src_stride + w0;
    uint64_t r = r0;
    if (D > 0) {
        for (; r + R <= r1; r += R, in += R * src_stride, out += R * dst_stride) {
            u64x2 v[R][D > 0 ? D : 1];
#pragma unroll
            for (int i = 0; i < R; i++)
#pragma unroll
                for (int j = 0; j < D; j++) v[i][j] = fold_load<NT>(in + i * src_stride + j * fold);
#pragma unroll
            for (int i = 0; i < R; i++) {
                u64x2 acc = v[i][0];
#pragma unroll
                for (int j = 1; j < D; j++) acc |= v[i][j];
                *reinterpret_cast<u64x2 *>(out + i * dst_stride) = acc & keep;
            }
        }
        for (; r < r1; r++, in += src_stride, out += dst_stride) {
            u64x2 v[D > 0 ? D : 1];
#pragma unroll
            for (int j = 0; j < D; j++) v[j] = fold_load<NT>(in + j * fold);
            u64x2 acc = v[0];
#pragma unroll
            for (int j = 1; j < D; j++) acc |= v[j];
            *reinterpret_cast<u64x2 *>(out) = acc & keep;
        }
    } else {
        for (; r < r1; r++, in += src_stride, out += dst_stride) {
            u64x2 acc{0ull, 0ull};
            const uint64_t *q = in;
            uint64_t j = 0;
            for (; j + L <= factor; j += L, q += L * fold) {
                u64x2 v[L];
#pragma unroll
                for (int t = 0; t < L; t++) v[t] = fold_load<NT>(q + t * fold);
#pragma unroll
                for (int t = 0; t < L; t++) acc |= v[t];
            }
            if (j < factor) {          // (wave-uniform)
                u64x2 v[L];
#pragma unroll
                for (int t = 0; t < L; t++) v[t] = j + t < factor ? fold_load<NT>(q + t * fold) : u64x2{0ull, 0ull};
#pragma unroll
                for (int t = 0; t < L; t++) acc |= v[t];
            }
            *reinterpret_cast<u64x2 *>(out) = acc & keep;
        }
    }
}

// ------------------------------------------------------------------------------ k-mer prevalence: per-k-mer sample counts
// For every unique k-mer of a batch, how many samples hold it: the popcount of the AND of its h rows over the whole width, under a
// mask -- the horizontal twin of k_col_popcount.  K1 of any route has left rows[slot * h .. +h), pos_off and num_unique behind; slot t
// of the batch's positions [0, total_pos) is a unique k-mer of its sequence q iff t - pos_off[q] < num_unique[q], and the other slots
// cost the search for q and that test.  Decomposition (plan_kmer_prevalence, bigsi_launch.hpp): wavefront w owns slice w % slices --
// the 1 KiB column segments [slice * segs_per_slice, +segs_per_slice) cut off at `segs` -- and the slots w / slices,
// + waves_per_slice, ...; a lane owns kVec words of a segment.  Everything that names a slot is wave-uniform (the wavefront's number
// goes through readfirstlane): the search of pos_off and the row ids are scalar loads, the row addresses scalar arithmetic, 64 bits
// wide (row x stride_words passes 2^32 on a 10 M-row index).
//   H > 0: h == H < kPrevLoads.  A step takes S = ceil(kPrevLoads / H) segments: S x H independent streamed 16-byte loads (8 to 14)
//          are in flight before the first AND.
//   H == 0: any h (the launcher sends h >= kPrevLoads here).  One segment at a time, its rows in groups of kPrevLoads independent
//          loads ANDed into a running value, the last group predicated (wave-uniform) on the rows that exist.
// A slice's whole steps run without a predicate; what is left of it is ONE more step in which a lane loads only the words below
// `wlim` = the end of the slice or of the words that carry columns (wv), whichever comes first: words from wv to the stride are not
// loaded, and a load of the word pair that holds word wv - 1 stays inside the row (the stride is a multiple of kVec words).
// `umask` is universe AND valid columns, `smask` subset AND umask, both built by the host in the row format (popcount is invariant
// under the format's bit permutation: no by_column anywhere), zero from the last column to segs x 128 words: the bits behind
// num_cols, which bigsi_hip_set_rows can put into the matrix, are never counted, and a mask load never leaves the buffer.  They are
// read by every wavefront and stay in L2 (plain loads).
// A lane counts into 32-bit accumulators (at most 128 x segs <= 2^26 per k-mer); at the end of the slice one wave reduction on the DPP
// path of the block scans, and the last lane stores the slice's partial -- one uint32, or {total, in_subset} as one 8-byte store --
// into partial[slice][slot].  Nobody else writes that entry and nobody reads an entry that was not written (k_kmer_prevalence_sum
// reads unique slots only): no atomics, no zeroed array, no LDS, no scratch, and no workgroup waits for another.
// Bounds: slot t < total_pos, so rows[t * h + j] is inside K1's array of total_pos x h ids, each < num_rows; a loaded word pair
// starts below wv <= stride_words.
__device__ __forceinline__ uint32_t wave_sum_last_lane(uint32_t v)      // lane 63 returns the sum over the wavefront
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);      // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);      // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);      // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);      // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);      // row_bcast:15 into rows 1 and 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);      // row_bcast:31 into rows 2 and 3
    return v;
}

// the sequence that owns position p: the largest q with pos_off[q] <= p (p < pos_off[n_seqs]; sequences without positions own none)
__device__ __forceinline__ uint32_t prevalence_owner(const uint64_t *__restrict__ pos_off, uint32_t n_seqs, uint64_t p)
{
    uint32_t lo = 0, hi = n_seqs;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pos_off[mid] <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

template <int H, bool SUBSET>
__global__ __launch_bounds__(kBlock) void k_kmer_prevalence(
    const uint64_t *__restrict__ index, uint64_t stride_words, uint64_t wv, const uint64_t *__restrict__ rows,
    const uint64_t *__restrict__ pos_off, const uint32_t *__restrict__ num_unique, uint32_t n_seqs, uint64_t total_pos, uint32_t h,
    const uint64_t *__restrict__ umask, const uint64_t *__restrict__ smask, uint32_t slices, uint32_t segs_per_slice, uint32_t segs,
    uint64_t waves_per_slice, uint32_t *__restrict__ partial, uint64_t partial_stride)
{
    constexpr int L = kPrevLoads, G = H > 0 ? H : L, S = H > 0 ? (L + H - 1) / H : 1;
    constexpr uint64_t SEG = 64 * kVec;          // words of a segment
    static_assert(H >= 0 && H < L && S * G <= kPrevMaxLoads, "plan_kmer_prevalence's invariant: at most kPrevMaxLoads loads per lane and step");
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wave >= waves_per_slice * slices) return;
    const uint32_t slice = (uint32_t)(wave % slices);
    const uint64_t s0 = (uint64_t)slice * segs_per_slice;
    const uint64_t s1 = s0 + segs_per_slice < segs ? s0 + segs_per_slice : segs;
    const uint64_t wlim = s1 * SEG < wv ? s1 * SEG : wv;

    for (uint64_t t = wave / slices; t < total_pos; t += waves_per_slice) {
        const uint32_t q = prevalence_owner(pos_off, n_seqs, t);
        if (t - pos_off[q] >= num_unique[q]) continue;          // a duplicate's slot: K1 left no rows here
        const uint64_t *__restrict__ rp = rows + t * h;
        uint64_t rid[G];
        if (H > 0) {
#pragma unroll
            for (int j = 0; j < G; j++) rid[j] = rp[j];
        }
        uint32_t tot = 0, sub = 0;
        auto count = [&](u64x2 a, uint64_t w) {
            const u64x2 u = *reinterpret_cast<const u64x2 *>(umask + w);
            tot += (uint32_t)__popcll(a.x & u.x) + (uint32_t)__popcll(a.y & u.y);
            if (SUBSET) {
                const u64x2 s = *reinterpret_cast<const u64x2 *>(smask + w);
                sub += (uint32_t)__popcll(a.x & s.x) + (uint32_t)__popcll(a.y & s.y);
            }
        };
        // the AND of all h rows at the lane's words [w, w + kVec) (H == 0: in groups of L loads)
        auto and_rows = [&](uint64_t w) {
            u64x2 a{~0ull, ~0ull};
            for (uint32_t g = 0; g < h; g += L) {
                u64x2 v[L];
#pragma unroll
                for (int j = 0; j < L; j++) v[j] = g + j < h ? load_row_seg(index, rp[g + j], stride_words, (uint32_t)w) : u64x2{~0ull, ~0ull};
#pragma unroll
                for (int j = 0; j < L; j++) a &= v[j];
            }
            return a;
        };
        uint64_t wb = s0 * SEG;          // first word of the step's first segment
        if (H > 0) {
            for (; wb + S * SEG <= wlim; wb += S * SEG) {
                u64x2 v[S][G];
#pragma unroll
                for (int i = 0; i < S; i++)
#pragma unroll
                    for (int j = 0; j < G; j++) v[i][j] = load_row_seg(index, rid[j], stride_words, (uint32_t)(wb + i * SEG + lane * kVec));
#pragma unroll
                for (int i = 0; i < S; i++) {
                    u64x2 a = v[i][0];
#pragma unroll
                    for (int j = 1; j < G; j++) a &= v[i][j];
                    count(a, wb + i * SEG + lane * kVec);
                }
            }
            if (wb < wlim) {          // (wave-uniform) the rest of the slice: fewer than S segments, the last one maybe part of one
                u64x2 v[S][G];
#pragma unroll
                for (int i = 0; i < S; i++) {
                    const uint64_t w = wb + i * SEG + lane * kVec;
#pragma unroll
                    for (int j = 0; j < G; j++) v[i][j] = w < wlim ? load_row_seg(index, rid[j], stride_words, (uint32_t)w) : u64x2{0ull, 0ull};
                }
#pragma unroll
                for (int i = 0; i < S; i++) {
                    const uint64_t w = wb + i * SEG + lane * kVec;
                    u64x2 a = v[i][0];
#pragma unroll
                    for (int j = 1; j < G; j++) a &= v[i][j];
                    if (w < wlim) count(a, w);
                }
            }
        } else {
            for (; wb + SEG <= wlim; wb += SEG) count(and_rows(wb + lane * kVec), wb + lane * kVec);
            if (wb + lane * kVec < wlim) count(and_rows(wb + lane * kVec), wb + lane * kVec);
        }
        tot = wave_sum_last_lane(tot);
        if (SUBSET) sub = wave_sum_last_lane(sub);
        if (lane == 63) {
            const uint64_t e = (uint64_t)slice * partial_stride + t;
            if (SUBSET) *reinterpret_cast<uint2 *>(partial + 2 * e) = uint2{tot, sub};
            else partial[e] = tot;
        }
    }
}

// A thread per POSITION p of the batch: out[p] = the sum over the slices of the partials of the position's unique k-mer, slot
// pos_off[q] + pos_unique[p] -- where duplicates are expanded, as the presence strings expand them.  `out_sub` non-null: the partials
// are {total, in_subset} pairs.
__global__ __launch_bounds__(kBlock) void k_kmer_prevalence_sum(
    const uint32_t *__restrict__ partial, uint64_t partial_stride, uint32_t slices, const uint64_t *__restrict__ pos_off, uint32_t n_seqs,
    const uint32_t *__restrict__ pos_unique, uint64_t total_pos, uint32_t *__restrict__ out_total, uint32_t *__restrict__ out_sub)
{
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= total_pos) return;
    const uint64_t slot = pos_off[prevalence_owner(pos_off, n_seqs, p)] + pos_unique[p];
    uint32_t tot = 0, sub = 0;
    for (uint32_t s = 0; s < slices; s++) {
        const uint64_t e = (uint64_t)s * partial_stride + slot;
        if (out_sub) {
            const uint2 v = *reinterpret_cast<const uint2 *>(partial + 2 * e);
            tot += v.x;
            sub += v.y;
        } else tot += partial[e];
    }
    out_total[p] = tot;
    if (out_sub) out_sub[p] = sub;
}

// ------------------------------------------------------------------------------ windowed search: the best window per sample
// found(c, s) = number of positions p in [s, s + We) whose k-mer's h rows all have bit c; per column the maximum over the window
// starts s (include/bigsi_hip_window.h).  K1 of any route has left rows[(pos_off[q] + u) * h .. +h) for the unique k-mers u of
// sequence q and pos_unique[pos_off[q] + p] = the unique k-mer of position p: a position's A_p is the AND of the h rows of ITS
// unique k-mer, so a repeated k-mer reuses a slot.
// k_window_max (launch shape: plan_window_search, bigsi_launch.hpp): a wavefront owns one segment [a, b) of window starts of one
// sequence and one tile of 64 x kVec column words; a lane owns kVec words, loaded 16 bytes at a time.  Per word it keeps two
// bit-sliced counters of P planes (P >= bit_width(We)): `cur` = found(., s) of all 64 columns at once, `best` = the running maximum.
//   warm-up  cur = sum of A_p over [a, a + We): k_and_count's ripple-carry add, 8 to 12 independent row loads in flight.
//   step     s -> s + 1: A_enter of position s + We, A_leave of position s; in = A_enter & ~A_leave is added (ripple carry), out =
//            A_leave & ~A_enter subtracted (ripple borrow).  No column has both, so cur never leaves [0, We].  A count grows only
//            where `in` has a bit: the compare-and-select from the top plane down (gt |= eq & cur & ~best; eq &= ~(cur ^ best);
//            best = gt ? cur : best) runs only when some lane of the wavefront has one (__ballot).  KM steps' 2 x KM x H loads are
//            issued together (8 to 14 in flight), then applied in order.
// Every plane array is indexed by compile-time constants in fully unrolled loops (registers, no scratch).  At the end the wavefront
// stores its P planes of `best`, bit-sliced as they are, as 16-byte stores to partial[(seg * P + plane) * wvp + w0]: nobody else
// writes that entry.  No atomics, no LDS, no scratch, and no workgroup waits for another.
// Bounds: positions touched are a .. b - 2 + We <= n - 1 (b <= n - We + 1), each mapped through pos_unique to a slot u < num_unique[q]
// <= n, so every slot index pos_off[q] + u is below total_pos and every row id below num_rows; the leaving position is s >= a.  A
// loaded word pair starts at w0 < wv <= stride_words, w0 even and the stride a multiple of kVec words, so it ends inside the row;
// words from wv to the stride are not loaded (the lane returns).  A stored pair ends at or before wvp = round_up(wv, kVec).
template <int P, int H>
__global__ __launch_bounds__(kBlock) void k_window_max(
    const uint64_t *__restrict__ index, uint64_t stride_words, uint32_t wv, const uint64_t *__restrict__ rows,
    const uint64_t *__restrict__ pos_off, const uint32_t *__restrict__ pos_unique, uint32_t h_rt, const WindowSeg *__restrict__ segs,
    uint64_t n_segs, uint32_t tiles, uint64_t *__restrict__ partial, uint64_t wvp)
{
    constexpr int HH = H > 0 ? H : 1;
    constexpr int KMW = H == 1 ? 8 : H <= 3 ? 4 : 2;          // warm-up positions per iteration
    constexpr int KM = H == 1 ? 4 : H <= 3 ? 2 : 1;           // window steps per iteration (window_steps_per_iter)
    const uint32_t h = H > 0 ? (uint32_t)H : h_rt;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = (uint64_t)blockIdx.x * (kBlock / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wave >= n_segs * tiles) return;
    const uint64_t seg = wave / tiles;
    const uint32_t tile = (uint32_t)(wave - seg * tiles);
    const uint32_t w0 = (tile * 64u + lane) * kVec;
    if (w0 >= wv) return;
    const uint32_t q = (uint32_t)__builtin_amdgcn_readfirstlane((int)segs[seg].q);
    const uint32_t a = (uint32_t)__builtin_amdgcn_readfirstlane((int)segs[seg].a);
    const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)segs[seg].b);
    const uint32_t we = (uint32_t)__builtin_amdgcn_readfirstlane((int)segs[seg].we);
    const uint64_t p0 = pos_off[q];
    const uint64_t *__restrict__ qrows = rows + p0 * h;
    const uint32_t *__restrict__ pu = pos_unique + p0;

    uint64_t cur[kVec][P], best[kVec][P];
#pragma unroll
    for (int e = 0; e < kVec; e++)
#pragma unroll
        for (int p = 0; p < P; p++) cur[e][p] = 0;

    auto add = [&](const RowWords<kVec> &x) {
        uint64_t c[kVec];
#pragma unroll
        for (int e = 0; e < kVec; e++) c[e] = x.word(e);
#pragma unroll
        for (int p = 0; p < P; p++) {
#pragma unroll
            for (int e = 0; e < kVec; e++) {
                const uint64_t t = cur[e][p] & c[e];
                cur[e][p] ^= c[e];
                c[e] = t;
            }
        }
    };
    auto step = [&](const RowWords<kVec> &enter, const RowWords<kVec> &leave) {
        uint64_t in[kVec], c[kVec], bw[kVec];
#pragma unroll
        for (int e = 0; e < kVec; e++) {
            in[e] = enter.word(e) & ~leave.word(e);
            c[e] = in[e];
            bw[e] = leave.word(e) & ~enter.word(e);
        }
#pragma unroll
        for (int p = 0; p < P; p++) {
#pragma unroll
            for (int e = 0; e < kVec; e++) {
                const uint64_t t = cur[e][p] & c[e];
                cur[e][p] ^= c[e];
                c[e] = t;
            }
        }
#pragma unroll
        for (int p = 0; p < P; p++) {
#pragma unroll
            for (int e = 0; e < kVec; e++) {
                const uint64_t t = ~cur[e][p] & bw[e];
                cur[e][p] ^= bw[e];
                bw[e] = t;
            }
        }
        uint64_t any = 0;
#pragma unroll
        for (int e = 0; e < kVec; e++) any |= in[e];
        if (__ballot(any != 0) == 0ull) return;
#pragma unroll
        for (int e = 0; e < kVec; e++) {
            uint64_t gt = 0, eq = ~0ull;
#pragma unroll
            for (int p = P - 1; p >= 0; p--) {
                gt |= eq & cur[e][p] & ~best[e][p];
                eq &= ~(cur[e][p] ^ best[e][p]);
            }
#pragma unroll
            for (int p = 0; p < P; p++) best[e][p] = (cur[e][p] & gt) | (best[e][p] & ~gt);
        }
    };
    // A_p of one position, its rows in groups of four loads (tails, and every position when h is a run-time value)
    auto and_rows = [&](uint32_t p) {
        const uint64_t *kr = qrows + (uint64_t)pu[p] * h;
        RowWords<kVec> x = RowWords<kVec>::fill(~0ull);
        uint32_t s = 0;
        for (; s + 4 <= h; s += 4) {
            RowWords<kVec> l0 = RowWords<kVec>::load(index, kr[s], stride_words, w0), l1 = RowWords<kVec>::load(index, kr[s + 1], stride_words, w0);
            const RowWords<kVec> l2 = RowWords<kVec>::load(index, kr[s + 2], stride_words, w0), l3 = RowWords<kVec>::load(index, kr[s + 3], stride_words, w0);
            l0 &= l2; l1 &= l3; l0 &= l1;
            x &= l0;
        }
        for (; s < h; s++) x &= RowWords<kVec>::load(index, kr[s], stride_words, w0);
        return x;
    };

    // warm-up: the window at start a
    uint32_t p = a;
    const uint32_t pe = a + we;
    if (H > 0) {
        for (; p + KMW <= pe; p += KMW) {
            RowWords<kVec> v[KMW * HH];
#pragma unroll
            for (int g = 0; g < KMW; g++) {
                const uint64_t *kr = qrows + (uint64_t)pu[p + g] * HH;
#pragma unroll
                for (int s = 0; s < HH; s++) v[g * HH + s] = RowWords<kVec>::load(index, kr[s], stride_words, w0);
            }
#pragma unroll
            for (int g = 0; g < KMW; g++) {
                RowWords<kVec> x = v[g * HH];
#pragma unroll
                for (int s = 1; s < HH; s++) x &= v[g * HH + s];
                add(x);
            }
        }
    }
    for (; p < pe; p++) add(and_rows(p));
#pragma unroll
    for (int e = 0; e < kVec; e++)
#pragma unroll
        for (int pp = 0; pp < P; pp++) best[e][pp] = cur[e][pp];

    // the steps a -> a + 1 -> ... -> b - 1
    uint32_t s = a;
    if (H > 0) {
        for (; s + KM < b; s += KM) {
            RowWords<kVec> ve[KM * HH], vl[KM * HH];
#pragma unroll
            for (int g = 0; g < KM; g++) {
                const uint64_t *ke = qrows + (uint64_t)pu[s + g + we] * HH, *kl = qrows + (uint64_t)pu[s + g] * HH;
#pragma unroll
                for (int t = 0; t < HH; t++) {
                    ve[g * HH + t] = RowWords<kVec>::load(index, ke[t], stride_words, w0);
                    vl[g * HH + t] = RowWords<kVec>::load(index, kl[t], stride_words, w0);
                }
            }
#pragma unroll
            for (int g = 0; g < KM; g++) {
                RowWords<kVec> xe = ve[g * HH], xl = vl[g * HH];
#pragma unroll
                for (int t = 1; t < HH; t++) { xe &= ve[g * HH + t]; xl &= vl[g * HH + t]; }
                step(xe, xl);
            }
        }
    }
    for (; s + 1 < b; s++) {
        const RowWords<kVec> xe = and_rows(s + we), xl = and_rows(s);
        step(xe, xl);
    }

    uint64_t *o = partial + seg * (uint64_t)P * wvp + w0;
#pragma unroll
    for (int pp = 0; pp < P; pp++) *reinterpret_cast<u64x2 *>(o + (uint64_t)pp * wvp) = u64x2{best[0][pp], best[kVec - 1][pp]};
}

// k_window_combine: a thread per (sequence, 64-column word): the per-column maximum over the sequence's segments (the same
// compare-and-select over the stored planes), thresholded against need[q] into the hit bitmap K4 compacts -- columns >= num_cols
// masked off, a sequence without segments (no k-mer position) all zero -- and, for words that hold a hit, expanded to uint16 counters
// in the layout k_and_count leaves (out[q * out_stride + column]): k_hits_totals / k_hits_write then build the hit lists unchanged.
template <int P>
__global__ __launch_bounds__(kBlock) void k_window_combine(
    const uint64_t *__restrict__ partial, uint64_t wvp, const uint64_t *__restrict__ seg_off, uint32_t n_seqs, uint32_t wv,
    uint32_t blocks_per_seq, const uint32_t *__restrict__ need, uint64_t n_cols, uint64_t *__restrict__ hit_bitmap, uint64_t bm_stride,
    uint16_t *__restrict__ out, uint64_t out_stride)
{
    const uint32_t q = blockIdx.x / blocks_per_seq, w = (blockIdx.x - q * blocks_per_seq) * kBlock + threadIdx.x;
    if (q >= n_seqs || w >= wv) return;
    const uint64_t s0 = seg_off[q], s1 = seg_off[q + 1];
    uint64_t best[P];
#pragma unroll
    for (int p = 0; p < P; p++) best[p] = 0;
    for (uint64_t s = s0; s < s1; s++) {
        uint64_t cur[P];
#pragma unroll
        for (int p = 0; p < P; p++) cur[p] = partial[(s * P + p) * wvp + w];
        uint64_t gt = 0, eq = ~0ull;
#pragma unroll
        for (int p = P - 1; p >= 0; p--) {
            gt |= eq & cur[p] & ~best[p];
            eq &= ~(cur[p] ^ best[p]);
        }
#pragma unroll
        for (int p = 0; p < P; p++) best[p] = (cur[p] & gt) | (best[p] & ~gt);
    }
    const uint32_t thr = need[q];
    uint64_t gt = 0, eq = ~0ull;
    if ((thr >> P) != 0) eq = 0;
#pragma unroll
    for (int p = P - 1; p >= 0; p--) {
        if ((thr >> p) & 1u) eq &= best[p];
        else { gt |= eq & best[p]; eq &= ~best[p]; }
    }
    const uint64_t ge = s0 < s1 ? (gt | eq) & valid_mask(w, n_cols) : 0ull;
    hit_bitmap[(uint64_t)q * bm_stride + w] = ge;
    if (ge == 0) return;
    // column 8b + jj of the word sits at bit 8b + 7 - jj; 8 consecutive counters per store
    uint16_t *o = out + (uint64_t)q * out_stride + (uint64_t)w * 64;
#pragma unroll
    for (int b = 0; b < 8; b++) {
        uint32_t c[8];
#pragma unroll
        for (int jj = 0; jj < 8; jj++) {
            const int bit = 8 * b + 7 - jj;
            uint32_t x = 0;
#pragma unroll
            for (int p = 0; p < P; p++) x |= (uint32_t)((best[p] >> bit) & 1ull) << p;
            c[jj] = x;
        }
        *reinterpret_cast<uint4 *>(o + 8 * b) = uint4{c[0] | (c[1] << 16), c[2] | (c[3] << 16), c[4] | (c[5] << 16), c[6] | (c[7] << 16)};
    }
}

// The second, independent route to a hit's record: its presence bits by position, then a walk over the window starts.
// k_window_bits: a wavefront per (hit, 64 positions): lane l tests position 64 blk + l of the hit's sequence -- bit c of the AND of
// the h words of the position's unique k-mer, 8-byte loads as k_presence makes them -- and the ballot is the word bits[g] (bit l =
// position 64 blk + l, zero behind the last position).  The words of the hits of sequence q start at word_off[q]; hit i of q (i from
// hit_off[q]) owns ceil(n / 64) of them.  Bounds: g < word_off[n_seqs] = the size of `bits`; positions p < n only.
__global__ __launch_bounds__(kBlock) void k_window_bits(
    const uint64_t *__restrict__ index, uint64_t stride_words, const uint64_t *__restrict__ rows, const uint64_t *__restrict__ pos_off,
    const uint32_t *__restrict__ pos_unique, const uint32_t *__restrict__ num_kmers, uint32_t h, uint32_t n_seqs,
    const uint64_t *__restrict__ word_off, const uint64_t *__restrict__ hit_off, const uint32_t *__restrict__ hit_col,
    uint64_t *__restrict__ bits)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t g = (uint64_t)blockIdx.x * (kBlock / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (g >= word_off[n_seqs]) return;
    const uint32_t q = prevalence_owner(word_off, n_seqs, g);
    const uint32_t n = num_kmers[q], words = (n + 63u) / 64u;
    const uint64_t r = g - word_off[q];
    const uint64_t hit = hit_off[q] + r / words;
    const uint32_t blk = (uint32_t)(r % words);
    const uint32_t c = hit_col[hit], p = blk * 64u + lane;
    bool present = false;
    if (p < n) {
        const uint64_t p0 = pos_off[q];
        const uint64_t *kr = rows + (p0 + pos_unique[p0 + p]) * h;
        uint64_t x = ~0ull;
        for (uint32_t s = 0; s < h; s++) x &= index[kr[s] * stride_words + (c >> 6)];
        present = ((x >> bit_of_col(c & 63u)) & 1ull) != 0;
    }
    const uint64_t word = __ballot(present);
    if (lane == 0) bits[g] = word;
}

struct WindowRecord {          // bigsi_hip_window_hit (include/bigsi_hip_window.h)
    uint32_t best_found, best_start, first_start, last_start, windows_passing, reserved;
};

// k_window_locate: a wavefront per hit over the hit's presence words.  Lane l takes the window starts [l C, (l + 1) C) of the
// sequence's n - We + 1, C = ceil(starts / 64) rounded up to a multiple of 64 (so that all lanes cross a word boundary in the same step): the first window's count from word popcounts, every further one from the running
// difference found += bit(s + We - 1) - bit(s - 1); it keeps the best count and its lowest start, the first and last start that
// reach need[q] and their number, and the wavefront reduces them over its lanes (shuffles; no LDS).  Its best_found shares no
// arithmetic with k_window_max's: the library compares the two on the host.
__global__ __launch_bounds__(kBlock) void k_window_locate(
    const uint64_t *__restrict__ bits, const uint64_t *__restrict__ word_off, const uint64_t *__restrict__ hit_off, uint32_t n_seqs,
    const uint32_t *__restrict__ num_kmers, const uint32_t *__restrict__ need, uint32_t window, WindowRecord *__restrict__ records)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t hit = (uint64_t)blockIdx.x * (kBlock / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (hit >= hit_off[n_seqs]) return;
    const uint32_t q = prevalence_owner(hit_off, n_seqs, hit);
    const uint32_t n = num_kmers[q], words = (n + 63u) / 64u, we = n < window ? n : window, thr = need[q];
    const uint64_t *__restrict__ B = bits + word_off[q] + (hit - hit_off[q]) * words;
    const uint32_t starts = n - we + 1u, per = ((starts + 63u) / 64u + 63u) & ~63u;          // a multiple of 64: every lane reloads its words in the same step
    const uint32_t lo = lane * per < starts ? lane * per : starts, hi = lo + per < starts ? lo + per : starts;
    uint32_t best = 0, best_s = 0xFFFFFFFFu, first = 0xFFFFFFFFu, last = 0, count = 0;
    if (lo < hi) {
        // found(lo): the bits [lo, lo + we) -- whole words, the two ends masked
        uint32_t found = 0;
        const uint32_t e = lo + we;                             // (exclusive; e <= n)
        for (uint32_t w = lo >> 6; w <= (e - 1u) >> 6; w++) {
            uint64_t x = B[w];
            if (w == lo >> 6) x &= ~0ull << (lo & 63u);
            if (w == (e - 1u) >> 6 && (e & 63u)) x &= ~0ull >> (64u - (e & 63u));
            found += (uint32_t)__popcll(x);
        }
        best = found;
        best_s = lo;
        if (found >= thr) { first = lo; last = lo; count = 1; }
        uint64_t win = 0, wout = 0;                             // the words of the entering and the leaving bit: one load per 64 steps
        for (uint32_t s = lo + 1u; s < hi; s++) {
            const uint32_t in = s + we - 1u, out = s - 1u;      // (in <= n - 1: s <= starts - 1)
            if ((in & 63u) == 0 || s == lo + 1u) win = B[in >> 6];
            if ((out & 63u) == 0 || s == lo + 1u) wout = B[out >> 6];
            found += (uint32_t)((win >> (in & 63u)) & 1ull);
            found -= (uint32_t)((wout >> (out & 63u)) & 1ull);
            if (found > best) { best = found; best_s = s; }
            if (found >= thr) {
                if (first == 0xFFFFFFFFu) first = s;
                last = s;
                count++;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t ob = (uint32_t)__shfl_xor((int)best, d, 64), os = (uint32_t)__shfl_xor((int)best_s, d, 64);
        const uint32_t of = (uint32_t)__shfl_xor((int)first, d, 64), ol = (uint32_t)__shfl_xor((int)last, d, 64);
        const uint32_t oc = (uint32_t)__shfl_xor((int)count, d, 64);
        if (ob > best || (ob == best && os < best_s)) { best = ob; best_s = os; }
        first = of < first ? of : first;
        last = ol > last ? ol : last;
        count += oc;
    }
    if (lane == 0) records[hit] = WindowRecord{best, best_s, first, last, count, 0u};
}

// transpose (bigsi/matrix/transpose.py:33-43) on the device: n Bloom filters (bloom c at blooms + c*bloom_stride, m bits,
// row byte format) become columns [col0, col0+n) of the matrix.  One thread per (row, 64-column word); the 8 threads of
// 8 consecutive rows read the same Bloom byte (one L1 line per wave), the word is read-modified-written once.
__global__ __launch_bounds__(kBlock) void k_insert_columns(
    uint64_t *__restrict__ index, uint64_t stride_words, uint64_t m, uint64_t col0, uint64_t ncols,
    const uint8_t *__restrict__ blooms, uint64_t bloom_stride)
{
    const uint64_t w0 = col0 >> 6, nwords = ((col0 + ncols - 1) >> 6) - w0 + 1;
    const uint64_t total = m * nwords;
    for (uint64_t item = (uint64_t)blockIdx.x * kBlock + threadIdx.x; item < total; item += (uint64_t)gridDim.x * kBlock) {
        const uint64_t r = item % m, w = w0 + item / m;
        const uint64_t clo = col0 > w * 64 ? col0 : w * 64;
        const uint64_t chi = col0 + ncols < w * 64 + 64 ? col0 + ncols : w * 64 + 64;
        uint64_t mask = 0, val = 0;
        for (uint64_t c = clo; c < chi; c++) {
            const uint64_t bit = (blooms[(c - col0) * bloom_stride + (r >> 3)] >> (7 - (r & 7))) & 1u;
            const uint32_t b = bit_of_col((uint32_t)(c & 63u));
            mask |= 1ull << b;
            val |= bit << b;
        }
        uint64_t *p = index + r * stride_words + w;
        *p = (*p & ~mask) | val;
    }
}

constexpr int kTransposeTile = 512, kTransposeSuper = 32;      // rows of a tile pass; supertile edge, in tiles

// ------------------------------------------------------------------------------ the transpose without lane butterflies (round 6)
// The lane-butterfly transpose of rounds 2-6 (k_transpose_tiles, since removed) spent ~90 vector instructions per 64 x 64 bit
// block on six exchange steps between lanes, and passed every tile through the LDS twice (in, block by block in place, out); with
// the filters at an aligned pitch the memory side of it moved 5.0-5.2 TB/s and the kernel 4.1-4.4 (profiles/r06_transpose_ab_aligned.txt: "no phase 2").  k_transpose_regs does the BIT
// level of the transpose between the REGISTERS of a thread and the BYTE level on the way out of the LDS:
//   1. a thread loads 16 bytes (128 rows) of EIGHT neighbouring filters -- columns 8 g .. 8 g + 7, the columns of ONE byte of
//      the rows -- and transposes the 8 x 8 bit blocks between its 8 registers, all 16 byte lanes at once: three steps of
//      shift + v_bfi on register pairs (192 vector instructions per 128 bytes, an eighth of the butterflies).  Register t then
//      holds, for each of the thread's 16 row-bytes e, the byte (columns 8 g .. 8 g + 7) of row 8 e + t;
//   2. it stores them as 8-byte words -- 8 bytes = 8 rows that are 8 apart, one column byte -- at LDS word (t, e / 8, p; g);
//   3. after ONE barrier, ds_read_b64_tr_b8 (gfx950's transposing LDS read: inside a group of 16 lanes, lane (a, b) receives byte
//      b of the words addressed by lanes 2 j + a, j = 0 .. 7; scripts/probe/tr_probe.hip prints the map read off the hardware)
//      hands every lane 8 CONSECUTIVE column bytes of one row: two reads = the 16 bytes of its store.  A wave instruction
//      stores 8 rows x 128 bytes.
// LDS: 64 x (128 + 4) words of 8 bytes = 66 KB per workgroup of 512 threads (512 rows x 1024 columns), two per CU; the +4
// words make the stores of phase 2 conflict-free (16 lanes = 4 column bytes x 4 pieces), the flip of word bit 3 by bit 5 the reads
// of phase 3 (32 lanes = 4 pieces x 8 column bytes, 16 words apart).
// RT = 2: 1024 rows per workgroup -- the thread loads both 64-byte halves of its filters' 128-byte lines at once and the two
// 512-row halves go through the LDS one after the other.
// 8 x 8 bit blocks between 8 registers, bytes independent: x[i] bit (7 - t) of byte q  ->  x[t] bit (7 - i) of byte q
__device__ __forceinline__ void transpose8_regs(uint32_t (&x)[8])
{
#define BIGSI_TR8_STEP(S, M)                                                                  \
    _Pragma("unroll") for (int u = 0; u < 8; u++) {                                           \
        if (u & S) continue;                                                                  \
        const uint32_t xu = x[u], xv = x[u + S];                                              \
        x[u + S] = (xv & (uint32_t)M) | ((xu << S) & ~(uint32_t)M);                           \
        x[u] = (xu & ~(uint32_t)M) | ((xv >> S) & (uint32_t)M);                               \
    }
    BIGSI_TR8_STEP(4, 0x0F0F0F0Fu)
    BIGSI_TR8_STEP(2, 0x33333333u)
    BIGSI_TR8_STEP(1, 0x55555555u)
#undef BIGSI_TR8_STEP
}

typedef int tr_v2i __attribute__((ext_vector_type(2)));

template <int RT, int CW = 1 /* tile width in units of 1024 columns: 2 = 256-byte row runs, 1024 threads, 133 KB of LDS (A/B) */>
__global__ __launch_bounds__(kBlock * 2 * CW) void k_transpose_regs(
    uint64_t *__restrict__ index, uint64_t stride_words, uint64_t m, uint64_t w_first /* first column word written; even */,
    uint64_t n_words /* 64-column words to write (all of each: columns at or beyond n_filters are written as zeros) */,
    const uint8_t *__restrict__ blooms /* filter of column 64 * w_first */, uint64_t n_filters /* filters there are, from that one on */,
    uint64_t bstride /* bytes between filters; multiple of 16 */, uint64_t nb /* valid bytes of a filter: ceil(m / 8) */,
    uint32_t rg, uint32_t cg /* tiles per XCD group along rows / columns: powers of two, rg * cg <= 128, cg <= sup_w */,
    uint32_t sup_w /* supertile width in tiles: a power of two <= 32 */)
{
    constexpr uint32_t kPitch = 128u * CW + 4u;           // 8-byte words per (t, eh, p) line of the image: the tile's column bytes + 4
    __shared__ __attribute__((aligned(16))) uint64_t image[64 * kPitch];
    constexpr uint32_t kWordsPerBlock = 16 * CW;        // 1024 CW columns
    auto word_at = [](uint32_t line, uint32_t cb) { return line * kPitch + (cb ^ ((cb >> 2) & 8u)); };
    // workgroup -> tile: supertiles of 1024 tiles, groups of rg x cg neighbours on one XCD
    const uint64_t tiles_c = (n_words + kWordsPerBlock - 1) / kWordsPerBlock, sup_c = (tiles_c + sup_w - 1) / sup_w;
    const uint32_t sup_h = (uint32_t)(kTransposeSuper * kTransposeSuper) / sup_w;
    const uint64_t sup = blockIdx.x / (kTransposeSuper * kTransposeSuper);
    const uint32_t within = blockIdx.x % (kTransposeSuper * kTransposeSuper);
    const uint32_t gsz = rg * cg, xcd = within & 7u, sl = within >> 3, tg = sl % gsz, grp = (sl / gsz) * 8u + xcd;
    const uint32_t gpr = sup_w / cg;
    const uint64_t tile_r = (sup / sup_c) * sup_h + (grp / gpr) * rg + tg % rg;
    const uint64_t tile_c = (sup % sup_c) * sup_w + (grp % gpr) * cg + tg / rg;
    if (tile_r * kTransposeTile * RT >= m || tile_c >= tiles_c) return;
    const uint64_t byte0 = tile_r * (kTransposeTile / 8) * RT;
    const uint64_t w0 = tile_c * kWordsPerBlock;
    const uint32_t words_here = (uint32_t)(n_words - w0 < kWordsPerBlock ? n_words - w0 : kWordsPerBlock);
    // phase 1: thread (g, p): 16 bytes at byte0 + 64 half + 16 p of the filters of columns 8 g .. 8 g + 7
    const uint32_t g = threadIdx.x >> 2, p = threadIdx.x & 3u;
    u64x2 ld[RT][8];
#pragma unroll
    for (int it = 0; it < 8; it++) {
#pragma unroll
        for (int half = 0; half < RT; half++) {
            const uint64_t off = byte0 + 64 * half + 16 * p;
            const bool ok = g < words_here * 8u && w0 * 64 + g * 8u + it < n_filters && off + 16 <= bstride && off < nb;
            const u64x2 *src = reinterpret_cast<const u64x2 *>(blooms + (w0 * 64 + (ok ? g * 8u + it : 0u)) * bstride + (ok ? off : 0));
            // PLAIN loads: the two 64-byte halves of a filter's line are asked for by consecutive instructions, and only a line the
            // vector L1 has allocated takes the second one as a hit -- with non-temporal loads the L2 was asked 1.19 times per line
            // (1.31 with RT = 1, where the other half belongs to another workgroup; TCC_EA0_RDREQ, scripts/pmc_requests.py), with the
            // halves eight instructions apart twice; with plain loads 1.000 (+5 ... +8 % on the kernel)
            ld[half][it] = ok ? *src : u64x2{0ull, 0ull};
        }
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    // phase 3's places: the wavefront takes the 64 rows 128 pw + 64 ehw + (0 .. 63) of the half; instruction t reads line (t, ehw, pw)
    // for the rows t + 8 b.  Lane = (gi, i): it ADDRESSES column byte 16 (2 gi + (i & 1)) + (i >> 1) (+ 8 for the second read) and
    // RECEIVES (b = i & 7, a = i >> 3) the bytes 16 (2 gi + a) + 0 .. 7 (8 .. 15) of row 8 b + t
    // (CW = 2: 16 wavefronts; a wavefront takes 4 of the 8 values of t and both 128-byte halves of its rows' 256-byte runs, one right after the other)
    const uint32_t pw = wave / (2u * CW), ehw = (wave / CW) & 1u, th = wave % CW, gi = lane >> 4, li = lane & 15u;
    const uint32_t cb_addr = 16u * (2u * gi + (li & 1u)) + (li >> 1);
    const uint32_t piece = 2u * gi + (li >> 3), brow = li & 7u;
#pragma unroll
    for (int half = 0; half < RT; half++) {
        if (half) __syncthreads();                          // phase 3 of the first half has read the image
        // phases 1b + 2: bit transpose between the registers, dword by dword, then the words of the image
#pragma unroll
        for (int d2 = 0; d2 < 2; d2++) {                    // d2 = eh: row bytes 16 p + 8 eh + (0 .. 7)
            uint32_t lo[8], hi[8];
#pragma unroll
            for (int it = 0; it < 8; it++) {
                const uint64_t v = d2 ? ld[half][it].y : ld[half][it].x;
                lo[it] = (uint32_t)v;
                hi[it] = (uint32_t)(v >> 32);
            }
            transpose8_regs(lo);
            transpose8_regs(hi);
#pragma unroll
            for (int t = 0; t < 8; t++) image[word_at((t * 2 + d2) * 4 + p, g)] = ((uint64_t)hi[t] << 32) | lo[t];
        }
        __syncthreads();
        const uint64_t r0 = (tile_r * RT + half) * kTransposeTile + 128u * pw + 64u * ehw + 8u * brow;
        tr_v2i v0[8], v1[8];
#pragma unroll
        for (int sl = 0; sl < 8; sl++) {                     // store slot sl = (t, 128-byte half of the run)
            const uint32_t t = (8u / CW) * th + sl / CW, ch = sl % CW, line = (t * 2 + ehw) * 4 + pw;
            v0[sl] = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) tr_v2i *)(image + word_at(line, 128u * ch + cb_addr)));
            v1[sl] = __builtin_amdgcn_ds_read_tr8_b64_v2i32((__attribute__((address_space(3))) tr_v2i *)(image + word_at(line, 128u * ch + cb_addr + 8u)));
        }
#pragma unroll
        for (int sl = 0; sl < 8; sl++) {
            const uint32_t t = (8u / CW) * th + sl / CW, pc = 8u * (sl % CW) + piece;
            const uint64_t r = r0 + t;
            if (r >= m || pc * 2 >= words_here) continue;
            const uint64_t a = ((uint64_t)(uint32_t)v0[sl].y << 32) | (uint32_t)v0[sl].x, b = ((uint64_t)(uint32_t)v1[sl].y << 32) | (uint32_t)v1[sl].x;
            uint64_t *dst = index + r * stride_words + w_first + w0 + pc * 2;
            // (non-temporal STORES stay: plain ones measured -2 ... -4 % on three shapes, three interleaved repetitions)
            if (pc * 2 + 1 < words_here) __builtin_nontemporal_store(u64x2{a, b}, reinterpret_cast<u64x2 *>(dst));
            else dst[0] = a;
        }
    }
}

// merge_indexes (bigsi/graph/index.py:54-60): append the n2 columns of src after the n1 columns of dst, row by row,
// device to device.  One thread per (row, destination byte); bits are MSB-first inside a byte, so a column offset that
// is not a multiple of 8 is a bit shift across source bytes.
__global__ __launch_bounds__(kBlock) void k_append_columns(
    uint64_t *__restrict__ dst, uint64_t dst_stride_words, uint64_t n1, const uint64_t *__restrict__ src, uint64_t src_stride_words,
    uint64_t n2, uint64_t m)
{
    // one thread per (row, destination word): in plain column order (by_column) the appended columns are the source row shifted
    // up by n1 % 64 bits -- two source words funnel into one destination word; the first destination word keeps its own
    // low columns.  (The first version moved one byte per thread, bit by bit.)
    const uint64_t j0 = n1 >> 6, j1 = (n1 + n2 + 63) >> 6, per_row = j1 - j0;
    const uint32_t sh = (uint32_t)(n1 & 63u);
    const uint64_t src_words = (n2 + 63) >> 6;
    const uint64_t total = m * per_row;
    for (uint64_t item = (uint64_t)blockIdx.x * kBlock + threadIdx.x; item < total; item += (uint64_t)gridDim.x * kBlock) {
        const uint64_t r = item / per_row, q = item % per_row, j = j0 + q;
        const uint64_t *sr = src + r * src_stride_words;
        const uint64_t cur = q < src_words ? by_column(sr[q]) : 0ull;
        uint64_t v;
        if (sh == 0) {
            v = cur;
        } else {
            const uint64_t prev = q > 0 ? by_column(sr[q - 1]) : 0ull;
            v = (prev >> (64u - sh)) | (cur << sh);
        }
        const uint64_t end = n1 + n2;                      // columns at or beyond it stay zero
        if (end < (j + 1) * 64) v &= (end & 63u) ? ((1ull << (end & 63u)) - 1) : ~0ull;
        uint64_t *d = dst + r * dst_stride_words + j;
        if (q == 0 && sh) v |= by_column(*d) & ((1ull << sh) - 1);
        *d = by_column(v);
    }
}

// Bloom-add k-mers to one sample column of the transposed matrix (bloom/bloomfilter.py:25-32 + graph/bigsi.py:151).
__global__ __launch_bounds__(kBlock) void k_insert_kmers(
    uint64_t *__restrict__ index, uint64_t stride_words, uint64_t m, uint32_t h, uint64_t col,
    const char *__restrict__ seqs, const uint64_t *__restrict__ seq_off, uint32_t k)
{
    const uint32_t q = blockIdx.x;
    const char *s = seqs + seq_off[q];
    const uint64_t len = seq_off[q + 1] - seq_off[q];
    const uint64_t n = len >= k ? len - k + 1 : 0;
    const uint64_t w = col >> 6, bitmask = 1ull << bit_of_col((uint32_t)(col & 63u));
    for (uint64_t i = threadIdx.x; i < n; i += kBlock) {
        KmerView v{s + i, k, use_revcomp(s + i, k)};
        for (uint32_t sd = 0; sd < h; sd++)
            atomicOr((unsigned long long *)(index + row_of_hash(murmur3_32(v, sd), m) * stride_words + w), (unsigned long long)bitmask);
    }
}

// BIGSI.bloom (graph/bigsi.py:150-155): u k-mers (k bytes each, packed) -> m-bit filter in the row byte format.
__global__ __launch_bounds__(kBlock) void k_bloom(
    uint32_t *__restrict__ bloom_words, uint64_t m, uint32_t h, const char *__restrict__ kmers, uint64_t u, uint32_t k, bool raw)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < u; i += (uint64_t)gridDim.x * kBlock) {
        const char *km = kmers + i * k;
        KmerView v{km, k, raw ? false : use_revcomp(km, k)};
        for (uint32_t sd = 0; sd < h; sd++) {
            const uint64_t r = row_of_hash(murmur3_32(v, sd), m);
            // byte r/8, mask 0x80 >> (r%8), addressed through little-endian 32-bit words
            atomicOr(&bloom_words[r >> 5], 1u << (8u * (uint32_t)((r >> 3) & 3u) + 7u - (uint32_t)(r & 7u)));
        }
    }
}

// synthetic contents: must match oracle/bigsi_oracle.c: orc_synth_word / orc_valid_mask bit for bit.
__global__ __launch_bounds__(kBlock) void k_fill_synth(
    uint64_t *__restrict__ index, uint64_t m, uint64_t stride_words, uint64_t n_cols, uint64_t seed, uint64_t shard, uint32_t draws)
{
    const uint64_t base = mix64(seed + shard * 0x632BE59BD9B4E019ull);
    const uint64_t pairs_per_row = stride_words / 2, total = m * pairs_per_row;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t r = i / pairs_per_row, w = (i - r * pairs_per_row) * 2;
        const uint64_t rk = mix64(base ^ (r * 0x9E3779B97F4A7C15ull));
        u64x2 v = {~0ull, ~0ull};
        for (uint32_t d = 0; d < draws; d++) {
            v.x &= mix64(rk + (w * 8 + d) * 0xD1B54A32D192ED03ull);
            v.y &= mix64(rk + ((w + 1) * 8 + d) * 0xD1B54A32D192ED03ull);
        }
        v.x &= valid_mask(w, n_cols);
        v.y &= valid_mask(w + 1, n_cols);
        *reinterpret_cast<u64x2 *>(index + r * stride_words + w) = v;
    }
}

// ------------------------------------------------------------------------------ pairwise popcounts: |column i AND column j| for lists of columns
// Three kernels per chunk of rows (plan_pairwise, bigsi_launch.hpp, says how the rows are cut and why).
//
// k_columns_to_planes: the selected columns of a chunk, transposed.  A wavefront owns the 64-row group g of the chunk (rows
// row0 + 64 g ..), a lane one row of it; planes[u * plane_stride + g] gets bit k = the bit of plane u's column in row row0 + 64 g + k.
// The planes are the distinct selected columns in ascending order, so the wavefront walks the distinct source words upwards
// (words / first / bit: pairwise_tables), kPlaneLoads 8-byte loads in flight per lane, and every selected column of a loaded word is
// one shift, one __ballot and one 8-byte store by lane 0.  The lanes of a load touch 64 rows, i.e. 64 lines, of which the next
// words of the same rows use the rest while they are in the cache.  A lane whose row is at or beyond num_rows loads nothing and
// contributes 0: rows an in-place fold left in the allocation are never counted, and a group wholly beyond num_rows is a zero word.
__global__ __launch_bounds__(kBlock) void k_columns_to_planes(
    const uint64_t *__restrict__ index, uint64_t stride_words, uint64_t num_rows, uint64_t row0, uint64_t groups,
    const uint32_t *__restrict__ words, const uint32_t *__restrict__ first, const uint32_t *__restrict__ bit, uint32_t num_words,
    uint64_t *__restrict__ planes, uint64_t plane_stride)
{
    const uint64_t g = (uint64_t)blockIdx.x * (kBlock / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (g >= groups) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t r = row0 + g * 64 + lane;
    const bool valid = r < num_rows;
    const uint64_t *row = index + (valid ? r : 0) * stride_words;
    for (uint32_t k0 = 0; k0 < num_words; k0 += kPlaneLoads) {
        uint64_t v[kPlaneLoads];
#pragma unroll
        for (int j = 0; j < kPlaneLoads; j++) v[j] = (valid && k0 + j < num_words) ? row[words[k0 + j]] : 0ull;
#pragma unroll
        for (int j = 0; j < kPlaneLoads; j++) {
            if (k0 + j >= num_words) break;
            const uint32_t u1 = first[k0 + j + 1];
            for (uint32_t u = first[k0 + j]; u < u1; u++) {
                const uint64_t word = __ballot((int)((v[j] >> bit[u]) & 1ull));
                if (lane == 0) planes[(uint64_t)u * plane_stride + g] = word;
            }
        }
    }
}

// k_pair_popcount: the tiled popcount "GEMM".  Workgroup (tile, slice): tile = (ti, tj) of kPairTile x kPairTile (distinct A column,
// distinct B column) pairs, slice = words [w_begin, w_end) of the chunk's planes.  Both plane tiles are staged kPairStageWords words
// at a time: a thread loads one 8-byte word (32 lanes = 256 consecutive bytes of one plane) and stores it at lds[word][column];
// columns beyond the list and words beyond the slice are staged as 0.  Thread (ty, tx) of 16 x 16 owns the pairs
// (pair_col(ty, a), pair_col(tx, b)), a, b < 4 -- two neighbouring columns in each half of the tile: per word it reads them as two
// 16-byte values per operand (ds_read_b128) and does, per pair, two 32-bit ANDs and two popcounts that add into the pair's 32-bit
// counter (v_bcnt_u32_b32 accumulates): 4 VALU operations per 64 pair-bits.
// LDS layout, stated for the reads of a wavefront (a ds_read_b128 is served in four groups of 16 lanes, banks = (address / 4) % 64):
// the word w of an operand is a run of kPairTile consecutive 64-bit values (kPairLdsStride = kPairTile + 2 apart from word to word:
// 16-byte aligned).  A group holds at most two values of ty and up to sixteen of tx: an A read is two addresses 16 bytes apart, each
// broadcast; a B read is sixteen consecutive 16-byte values = the 64 banks once.  Both are conflict-free.  The pad only serves the
// staging stores.  (The first version read eight 8-byte values per word at a stride of 16 columns; the compiler paired them into
// ds_read2_b64, half the bytes per LDS clock: DESIGN.md section 3 has both measurements.)
// A counter sees at most 64 (w_end - w_begin) <= 2^30 rows.  Symmetric calls: the workgroups of tiles tj < ti leave at once, the
// sum reads the mirror.  partial[slice][ua][ub]: nua x nub 32-bit counts per slice, no padding (stores are guarded).
// the k-th of the kPairReg tile columns thread coordinate t (0 .. 15) owns: 2 t, 2 t + 1, 32 + 2 t, 32 + 2 t + 1
__device__ __forceinline__ uint32_t pair_col(uint32_t t, int k) { return 2u * t + (uint32_t)(k & 1) + 32u * (uint32_t)(k >> 1); }

__global__ __launch_bounds__(kBlock) void k_pair_popcount(
    const uint64_t *__restrict__ planes, uint64_t plane_stride, uint64_t chunk_words, uint64_t slice_words,
    const uint32_t *__restrict__ plane_a, uint32_t nua, const uint32_t *__restrict__ plane_b, uint32_t nub, uint32_t tiles_j, uint32_t symmetric,
    uint32_t *__restrict__ partial)
{
    __shared__ __attribute__((aligned(16))) uint64_t lds_a[kPairStageWords * kPairLdsStride], lds_b[kPairStageWords * kPairLdsStride];
    const uint32_t ti = blockIdx.x / tiles_j, tj = blockIdx.x % tiles_j;
    if (symmetric && tj < ti) return;
    const uint64_t w_begin = (uint64_t)blockIdx.y * slice_words, w_end = min(w_begin + slice_words, chunk_words);
    const uint32_t t = threadIdx.x, ty = t >> 4, tx = t & 15u;
    const uint32_t sw = t % kPairStageWords, sc = t / kPairStageWords;          // staging: this thread's word and first column
    constexpr uint32_t kPass = kBlock / kPairStageWords;                          // columns staged per pass
    uint32_t acc[kPairReg][kPairReg] = {};
    for (uint64_t w0 = w_begin; w0 < w_end; w0 += kPairStageWords) {
        const uint32_t nw = (uint32_t)min<uint64_t>(kPairStageWords, w_end - w0);
        __syncthreads();          // (the previous stage has been read)
#pragma unroll
        for (uint32_t c = sc; c < (uint32_t)kPairTile; c += kPass) {
            const uint32_t ia = ti * kPairTile + c, ib = tj * kPairTile + c;
            lds_a[sw * kPairLdsStride + c] = (sw < nw && ia < nua) ? planes[(uint64_t)plane_a[ia] * plane_stride + w0 + sw] : 0ull;
            lds_b[sw * kPairLdsStride + c] = (sw < nw && ib < nub) ? planes[(uint64_t)plane_b[ib] * plane_stride + w0 + sw] : 0ull;
        }
        __syncthreads();
        for (uint32_t w = 0; w < nw; w++) {
            uint64_t a[kPairReg], b[kPairReg];
#pragma unroll
            for (int i = 0; i < kPairReg; i += 2) {
                const u64x2 va = *reinterpret_cast<const u64x2 *>(&lds_a[w * kPairLdsStride + 2 * ty + 16 * i]);
                const u64x2 vb = *reinterpret_cast<const u64x2 *>(&lds_b[w * kPairLdsStride + 2 * tx + 16 * i]);
                a[i] = va.x; a[i + 1] = va.y;
                b[i] = vb.x; b[i + 1] = vb.y;
            }
#pragma unroll
            for (int i = 0; i < kPairReg; i++)
#pragma unroll
                for (int j = 0; j < kPairReg; j++) {
                    const uint64_t x = a[i] & b[j];
                    acc[i][j] = __popc((uint32_t)(x >> 32)) + (__popc((uint32_t)x) + acc[i][j]);
                }
        }
    }
    uint32_t *out = partial + (uint64_t)blockIdx.y * nua * nub;
#pragma unroll
    for (int i = 0; i < kPairReg; i++) {
        const uint32_t ia = ti * kPairTile + pair_col(ty, i);
#pragma unroll
        for (int j = 0; j < kPairReg; j++) {
            const uint32_t ib = tj * kPairTile + pair_col(tx, j);
            if (ia < nua && ib < nub) out[(uint64_t)ia * nub + ib] = acc[i][j];
        }
    }
}

// k_pair_popcount_sum: out[i][j] (64-bit, na x nb) gets -- `add` == 0, the first chunk -- or is increased by the sum over the chunk's
// slices of partial[slice][map_a[i]][map_b[j]]: list positions that repeat a column read the same count.  Symmetric calls
// (map_b == map_a, nub == nua) take a pair whose tile lies below the diagonal from the mirror tile, which k_pair_popcount did run.
__global__ __launch_bounds__(kBlock) void k_pair_popcount_sum(
    const uint32_t *__restrict__ partial, uint64_t slices, uint32_t nua, uint32_t nub, const uint32_t *__restrict__ map_a, uint64_t na,
    const uint32_t *__restrict__ map_b, uint64_t nb, uint32_t symmetric, uint32_t add, uint64_t *__restrict__ out)
{
    const uint64_t total = na * nb, per_slice = (uint64_t)nua * nub;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (uint64_t)gridDim.x * kBlock) {
        uint32_t u = map_a[e / nb], v = map_b[e % nb];
        if (symmetric && v / kPairTile < u / kPairTile) { const uint32_t s = u; u = v; v = s; }
        const uint32_t *p = partial + (uint64_t)u * nub + v;
        uint64_t s = 0;
        for (uint64_t k = 0; k < slices; k++) s += p[k * per_slice];
        out[e] = add ? out[e] + s : s;
    }
}

// ------------------------------------------------------------------------------ calibration: what this box gives bare row streams
// bigsi_hip_probe_rows (MEASUREMENT): a kernel with NO BIGSI code reads row lists of the index itself the way the row-AND
// kernels do -- one wavefront per 1 KiB column segment of every row of a "query", lane = 16 bytes, eight non-temporal loads in
// flight, AND-reduce -- so that a bench line can say which fraction of THIS box's random-row (counting kernel) or
// address-ordered (exact kernel) rate a leg reached: boxes differ by several per cent at identical clocks.
// ids: random = uniform over [0, m); sorted = one uniform draw per stratum [i*m/R, (i+1)*m/R): ascending by construction.
__global__ __launch_bounds__(kBlock) void k_probe_ids(uint64_t *__restrict__ ids, uint64_t n_queries, uint32_t rows_per_query, uint64_t m, uint32_t sorted, uint64_t seed)
{
    const uint64_t total = n_queries * rows_per_query;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (uint64_t)gridDim.x * kBlock) {
        const uint64_t r = mix64(seed + i * 0x9E3779B97F4A7C15ull);
        if (!sorted) {
            ids[i] = r % m;
        } else {
            const uint64_t j = i % rows_per_query, lo = (unsigned __int128)j * m / rows_per_query, hi = (unsigned __int128)(j + 1) * m / rows_per_query;
            ids[i] = lo + (hi > lo ? r % (hi - lo) : 0);
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_probe_rows(const uint64_t *__restrict__ index, uint64_t stride_words, uint32_t wv, const uint64_t *__restrict__ ids,
                                                       uint32_t rows_per_query, uint32_t segs, uint32_t q0, uint32_t q1, u64x2 *__restrict__ out)
{
    // (the wavefront's number is wave-uniform, which the compiler cannot see in threadIdx.x >> 6: without the readfirstlane the row
    // ids arrive through per-lane vector loads instead of scalar loads -- 6 % of the probe's rate; scripts/probe/row_probe.hip has
    // that handicap, which is why round 3's "bare kernel" figures sat BELOW k_and_exact)
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6))), lane = threadIdx.x & 63u;
    const uint32_t q = q0 + wave / segs, seg = wave % segs;
    if (q >= q1) return;
    const uint32_t w0 = seg * 128u + lane * kVec;
    if (w0 >= wv) return;
    const uint64_t *r = ids + (uint64_t)q * rows_per_query;
    u64x2 acc = {~0ull, ~0ull};
    uint32_t i = 0;
    for (; i + 8 <= rows_per_query; i += 8) {
        u64x2 v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = load_row_seg<true>(index, r[i + j], stride_words, w0);
#pragma unroll
        for (int j = 0; j < 8; j++) acc &= v[j];
    }
    for (; i < rows_per_query; i++) acc &= load_row_seg<true>(index, r[i], stride_words, w0);
    out[((uint64_t)(q - q0) * segs + seg) * 64 + lane] = acc;
}

// ------------------------------------------------------------------------------ query-set tally: per-sample hit totals of a batch
// The vertical sum over the result vectors a run made with BIGSI_RUN_SKIP_COMPACT left behind: queries_hit[s] += 1 and kmers_found[s]
// += c_q[s] for every query q whose bit of sample s is set (the AND of an exact run; count >= min_kmers of a counting run).  No hit
// list is built and nothing is compacted.
//
// k_tally_hits (launch shape: plan_tally).  A wavefront owns result word w -- 64 columns, lane l the column 64 w + l, whose bit in
// the word is bit_of_col(l), as K4 reads it (k_hits_write) -- and the queries [q0, q1) of one tile; the wavefronts of a workgroup own
// neighbouring words of the same tile.  Per query ONE wave-uniform 8-byte load of the word, kTallyLoads of them in flight, ANDed with
// valid_mask: bits behind num_cols are never trusted, and only words < wv are read (never the pad word of wv_pad).  A zero word --
// nearly all of them in a hit-sparse stream -- is skipped in a uniform branch before anything else of the query is touched.  Otherwise
// the query's num_unique (uniform; 0: the query has no k-mers and counts nowhere, whatever its vector holds), and every lane whose bit
// is set adds 1 and its k-mers: num_unique on the exact path (EXACT: counters is never read), its own counter on the counting path (a
// predicated load: the word's 64 counters are contiguous, one or two 128-byte lines per wavefront; in sparse mode the counters of a
// word that holds a hit are valid).  The sums stay in registers over the tile; then every lane with a non-zero sum issues one 64-bit
// atomic per accumulator, contiguous over the wavefront: a pair per column and WORKGROUP, never per query.  Integer sums: the result
// does not depend on the order the atomics arrive in.
template <typename CountT, bool EXACT>
__global__ __launch_bounds__(kBlock) void k_tally_hits(
    const uint64_t *__restrict__ bitmaps, uint64_t bm_stride, uint32_t wv, uint64_t n_cols, uint32_t n_seqs,
    const uint32_t *__restrict__ num_unique, const CountT *__restrict__ counters, uint64_t counter_stride, uint32_t word_groups, uint32_t tile,
    unsigned long long *__restrict__ queries_hit, unsigned long long *__restrict__ kmers_found)
{
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const uint32_t t = blockIdx.x / word_groups, w = (blockIdx.x - t * word_groups) * (kBlock / 64) + wave;
    if (w >= wv) return;
    const uint64_t vm = valid_mask(w, n_cols);
    const uint64_t q0 = (uint64_t)t * tile, q1 = q0 + tile < n_seqs ? q0 + tile : n_seqs;
    const uint32_t bit = bit_of_col(lane);
    uint32_t hits = 0;
    unsigned long long found = 0;
    for (uint64_t q = q0; q < q1; q += kTallyLoads) {
        uint64_t x[kTallyLoads];
#pragma unroll
        for (uint32_t j = 0; j < kTallyLoads; j++) x[j] = q + j < q1 ? bitmaps[(q + j) * bm_stride + w] & vm : 0ull;
#pragma unroll
        for (uint32_t j = 0; j < kTallyLoads; j++) {
            if (x[j] == 0) continue;
            const uint32_t u = num_unique[q + j];
            if (u == 0) continue;
            const bool mine = (x[j] >> bit) & 1ull;
            hits += mine ? 1u : 0u;
            if (EXACT) found += mine ? u : 0u;
            else if (mine) found += counters[(q + j) * counter_stride + (uint64_t)w * 64 + lane];
        }
    }
    if (hits) atomicAdd(&queries_hit[(uint64_t)w * 64 + lane], (unsigned long long)hits);
    if (found) atomicAdd(&kmers_found[(uint64_t)w * 64 + lane], found);
}

// k_tally_totals: totals[0] += queries with k-mers, [1] += their unique k-mers, [2] += queries without, [3] += queries with k-mers and
// at least one hit.  A workgroup owns kTallyTotalsTile queries, a wavefront every fourth of them (one each at the committed tile: the
// sweep of a query's words is a chain of load latencies, so the queries are spread over as many wavefronts as there are): the lanes OR the
// query's wv words (under valid_mask, kTallyLoads loads in flight) and the wavefront votes; the four wavefronts' sums meet in LDS and four
// threads issue one atomic each.
__global__ __launch_bounds__(kBlock) void k_tally_totals(
    const uint64_t *__restrict__ bitmaps, uint64_t bm_stride, uint32_t wv, uint64_t n_cols, uint32_t n_seqs,
    const uint32_t *__restrict__ num_unique, unsigned long long *__restrict__ totals)
{
    __shared__ unsigned long long lds[kBlock / 64][4];
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const uint64_t q0 = (uint64_t)blockIdx.x * kTallyTotalsTile, q1 = q0 + kTallyTotalsTile < n_seqs ? q0 + kTallyTotalsTile : n_seqs;
    unsigned long long counted = 0, unique = 0, skipped = 0, with_hits = 0;
    for (uint64_t q = q0 + wave; q < q1; q += kBlock / 64) {
        const uint32_t u = num_unique[q];
        if (u == 0) { skipped++; continue; }
        counted++;
        unique += u;
        uint64_t any = 0;
        for (uint32_t w0 = lane; w0 < wv; w0 += 64 * kTallyLoads) {          // kTallyLoads independent loads in flight per lane
            uint64_t x[kTallyLoads];
#pragma unroll
            for (uint32_t j = 0; j < kTallyLoads; j++) x[j] = w0 + 64 * j < wv ? bitmaps[q * bm_stride + w0 + 64 * j] : 0ull;
#pragma unroll
            for (uint32_t j = 0; j < kTallyLoads; j++) any |= x[j] & valid_mask(w0 + 64 * j, n_cols);
        }
        if (__ballot((int)(any != 0))) with_hits++;
    }
    if (lane == 0) { lds[wave][0] = counted; lds[wave][1] = unique; lds[wave][2] = skipped; lds[wave][3] = with_hits; }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long s = 0;
#pragma unroll
        for (int i = 0; i < kBlock / 64; i++) s += lds[i][threadIdx.x];
        if (s) atomicAdd(&totals[threadIdx.x], s);
    }
}

// ------------------------------------------------------------------------------ read classification: per-query verdicts over sample groups
// The horizontal sum over the result vectors a run made with BIGSI_RUN_SKIP_COMPACT left behind (include/bigsi_hip_classify.h has the
// definition): per query and group of columns how many columns are hit, the largest count among them and the lowest colour that
// holds it; out of the device go the two best groups, twelve uint32 per query.
//
// k_classify_groups (launch shape: plan_classify): ONE workgroup per query.
//   pass 1  the threads OR the query's wv words (thread = word: coalesced, kTallyLoads loads in flight) under valid_mask -- bits behind
//           num_cols are never trusted, the pad word of wv_pad is never read.  A query without k-mers, or without a set bit -- nearly
//           all of a hit-sparse stream --, writes its empty record and leaves before any LDS table is touched.
//   table   dynamic LDS, zeroed: best[n_groups] (uint64: found << 32 | 0xFFFFFFFF - colour, so that ONE integer max yields the largest
//           count and, among its columns, the lowest colour) | hits[n_groups] (uint32) | the wavefronts' partial results.
//   pass 2  a wavefront reads 64 words again (from L2), votes on the non-zero ones and takes them one after the other in the tally's
//           layout: lane l = column 64 w + l, bit bit_of_col(l).  A lane whose bit is set loads its group_of entry and, on the
//           counting path, its counter (both contiguous over the wavefront; in sparse mode all 64 counters of a word that holds a hit
//           are valid; EXACT: counters is never read, a hit has found = num_unique), and in a group issues an LDS add on hits[g] and an
//           LDS 64-bit max on best[g].
//   reduce  after a barrier every thread scans groups g = t, t + kBlock, ... for its two best keys found << 32 | 0xFFFFFFFF - g (found
//           descending, ties to the lower id; 0: none) and its number of hit groups; a butterfly over the wavefront, the wavefronts'
//           results through LDS, and thread 0 writes the record.
// Integer add and max only, no global atomic: the record does not depend on the order anything arrives in.
constexpr uint32_t kClassifyNone = 0xFFFFFFFFu;       // BIGSI_CLASSIFY_NONE (include/bigsi_hip_classify.h)

__device__ __forceinline__ void classify_merge(unsigned long long &a1, unsigned long long &a2, unsigned long long b1, unsigned long long b2)
{
    const unsigned long long lo = a1 < b1 ? a1 : b1, hi2 = a2 > b2 ? a2 : b2;
    a1 = a1 > b1 ? a1 : b1;
    a2 = lo > hi2 ? lo : hi2;
}

template <typename CountT, bool EXACT>
__global__ __launch_bounds__(kBlock) void k_classify_groups(
    const uint64_t *__restrict__ bitmaps, uint64_t bm_stride, uint32_t wv, uint64_t n_cols, const uint32_t *__restrict__ num_unique, double threshold,
    const CountT *__restrict__ counters, uint64_t counter_stride, const uint32_t *__restrict__ group_of, uint32_t n_groups, uint32_t table_bytes,
    uint4 *__restrict__ records)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    unsigned long long *best = reinterpret_cast<unsigned long long *>(smem);
    uint32_t *hits = reinterpret_cast<uint32_t *>(smem + (size_t)n_groups * 8);
    unsigned long long *part = reinterpret_cast<unsigned long long *>(smem + table_bytes);      // [kBlock / 64][3]: key1, key2, groups | samples
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const uint64_t q = blockIdx.x;
    const uint64_t *bm = bitmaps + q * bm_stride;
    uint4 *rec = records + q * 3;
    const uint32_t u = num_unique[q];
    const double mkd = ceil((double)u * threshold);          // min_kmers as K1 computes it
    const uint32_t mk = mkd > 0.0 ? (uint32_t)mkd : 0u;
    uint64_t any = 0;
    if (u)
        for (uint32_t w0 = threadIdx.x; w0 < wv; w0 += kBlock * kTallyLoads) {
            uint64_t x[kTallyLoads];
#pragma unroll
            for (uint32_t j = 0; j < kTallyLoads; j++) x[j] = w0 + kBlock * j < wv ? bm[w0 + kBlock * j] : 0ull;
#pragma unroll
            for (uint32_t j = 0; j < kTallyLoads; j++) any |= x[j] & valid_mask(w0 + kBlock * j, n_cols);
        }
    if (!__syncthreads_or((int)(any != 0))) {
        if (threadIdx.x == 0) {
            rec[0] = make_uint4(u, u ? mk : 0u, 0u, 0u);
            rec[1] = make_uint4(kClassifyNone, 0u, kClassifyNone, 0u);
            rec[2] = make_uint4(kClassifyNone, 0u, kClassifyNone, 0u);
        }
        return;
    }
    for (uint32_t g = threadIdx.x; g < n_groups; g += kBlock) { best[g] = 0ull; hits[g] = 0u; }
    __syncthreads();
    const uint32_t bit = bit_of_col(lane);
    uint32_t samples = 0;                                    // hit columns in any group, counted once per wavefront (uniform)
    for (uint32_t base = wave * 64; base < wv; base += kBlock) {
        const uint32_t w0 = base + lane;
        const uint64_t x = w0 < wv ? bm[w0] & valid_mask(w0, n_cols) : 0ull;
        uint64_t todo = __ballot((int)(x != 0));
        while (todo) {
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint64_t xw = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), src) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, src);
            const uint64_t col = (uint64_t)(base + (uint32_t)src) * 64 + lane;          // < n_cols wherever the bit is set (valid_mask)
            const bool mine = (xw >> bit) & 1ull;
            const uint32_t g = mine ? group_of[col] : kClassifyNone;
            const bool grouped = g != kClassifyNone;
            samples += (uint32_t)__popcll(__ballot((int)grouped));
            if (grouped) {
                const uint32_t found = EXACT ? u : (uint32_t)counters[q * counter_stride + col];
                atomicAdd(&hits[g], 1u);
                atomicMax(&best[g], ((unsigned long long)found << 32) | (0xFFFFFFFFu - (uint32_t)col));
            }
        }
    }
    __syncthreads();
    unsigned long long k1 = 0, k2 = 0;
    uint32_t groups = 0;
    for (uint32_t g = threadIdx.x; g < n_groups; g += kBlock)
        if (hits[g]) {
            groups++;
            classify_merge(k1, k2, (best[g] & 0xFFFFFFFF00000000ull) | (0xFFFFFFFFu - g), 0ull);
        }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o1 = __shfl_xor(k1, d), o2 = __shfl_xor(k2, d);
        classify_merge(k1, k2, o1, o2);
        groups += __shfl_xor(groups, d);
    }
    if (lane == 0) { part[wave * 3] = k1; part[wave * 3 + 1] = k2; part[wave * 3 + 2] = ((unsigned long long)groups << 32) | samples; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t samples_all = 0;
        groups = 0;
        k1 = k2 = 0;
        for (uint32_t i = 0; i < kBlock / 64; i++) {
            classify_merge(k1, k2, part[i * 3], part[i * 3 + 1]);
            groups += (uint32_t)(part[i * 3 + 2] >> 32);
            samples_all += (uint32_t)part[i * 3 + 2];
        }
        uint4 place[2];
        const unsigned long long key[2] = {k1, k2};
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const uint32_t g = 0xFFFFFFFFu - (uint32_t)key[i];
            place[i] = key[i] ? make_uint4(g, (uint32_t)(best[g] >> 32), 0xFFFFFFFFu - (uint32_t)best[g], hits[g])
                              : make_uint4(kClassifyNone, 0u, kClassifyNone, 0u);
        }
        rec[0] = make_uint4(u, mk, groups, samples_all);
        rec[1] = place[0];
        rec[2] = place[1];
    }
}

// ------------------------------------------------------------------------------ group association: per-query sample counts per group
// The hit-dense sibling of the classification (include/bigsi_hip_associate.h has the definition): per query and group of columns how
// many columns are hit -- every group's count, the zeros included.  No work per hit: a result word is ANDed with one mask word per
// group and popcounted, so the cost is the same whether a query hits nothing or every column.
//
// k_group_masks (one wavefront per result word w): group_of -> masks[n_groups][wv] in the bit layout K4 and the tally read -- lane l
//   of word w is column 64 w + l at bit bit_of_col(l).  bit_of_col is its own inverse, so the lane takes the column whose bit it is
//   (64 w + bit_of_col(lane): the same 256 contiguous bytes of group_of) and __ballot(group == g) is the mask word as stored.  A column
//   at or behind num_cols, or in no group, is set in no mask: valid_mask is implicit in every group count.
// k_group_counts (launch shape: plan_associate): a workgroup takes Q = kAssociateQueries = 4 queries; n_groups is taken in passes of
//   GB = kAssociateGroupBlock = 8 groups.  In a pass thread t sweeps words w = t, t + kBlock, ...: GB mask words and Q result words
//   (12 independent 8-byte loads; the masks from L2, shared by every workgroup; a result word from HBM in the first pass, from L2 in
//   the later ones) feed Q x GB popcounts into 32 register accumulators -- a mask word is loaded once for four queries, which is
//   what Q = 4 is for; GB = 8 keeps the accumulators, the masks and the result words of an iteration in 60 registers (the kernel
//   takes 93 VGPRs in all, no scratch, no spill).  The first pass also counts popcount(x & valid_mask(w, n_cols)) per query:
//   samples_hit.  Never w >= wv: the pad word of wv_pad is not read.  A query with num_unique == 0 (or behind n_seqs) loads nothing
//   and counts nothing.
//   reduce  the 32 accumulators of a wavefront by a halving exchange: in the step at distance d a lane keeps one half of its values,
//           sends the other half to lane ^ d and adds what it receives -- 16 + 8 + 4 + 2 + 1 shuffles, then one more over the last
//           pair, instead of 32 x 6 -- and lane 2 j holds the wavefront's sum of accumulator j; through static LDS to the
//           workgroup's sums; thread q * GB + g stores counts[q0 + q][g0 + g] plainly, and thread q < Q keeps the query's running
//           grouped_hit over the passes and writes the info behind the last.
// Integer AND, popcount and add only; no atomic anywhere, no early exit: the one sweep per pass is the whole cost.
__global__ __launch_bounds__(kBlock) void k_group_masks(const uint32_t *__restrict__ group_of, uint64_t n_cols, uint32_t wv, uint32_t n_groups,
                                                        uint64_t *__restrict__ masks)
{
    const uint32_t w = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (w >= wv) return;                                     // (uniform over the wavefront)
    const uint64_t col = (uint64_t)w * 64 + bit_of_col(lane);
    const uint32_t mine = col < n_cols ? group_of[col] : kAssociateNoGroup;
    for (uint32_t g = 0; g < n_groups; g++) {
        const uint64_t m = __ballot((int)(mine == g));
        if (lane == 0) masks[(uint64_t)g * wv + w] = m;
    }
}

// one step of the halving exchange at distance 2 N over acc[0 .. 2 N), and the steps below it (every index a constant: registers)
template <uint32_t N>
__device__ __forceinline__ void group_halve(uint32_t (&acc)[kAssociateQueries * kAssociateGroupBlock], uint32_t lane)
{
    const bool upper = (lane & (2 * N)) != 0;
#pragma unroll
    for (uint32_t i = 0; i < N; i++) {
        const uint32_t send = upper ? acc[i] : acc[i + N], keep = upper ? acc[i + N] : acc[i];
        acc[i] = keep + __shfl_xor(send, (int)(2 * N));
    }
    if constexpr (N > 1) group_halve<N / 2>(acc, lane);
}

__global__ __launch_bounds__(kBlock) void k_group_counts(
    const uint64_t *__restrict__ bitmaps, uint64_t bm_stride, uint32_t wv, uint64_t n_cols, const uint32_t *__restrict__ num_unique, double threshold,
    uint32_t n_seqs, const uint64_t *__restrict__ masks, uint32_t n_groups, uint32_t *__restrict__ counts, uint4 *__restrict__ info)
{
    constexpr uint32_t Q = kAssociateQueries, GB = kAssociateGroupBlock, NV = Q * GB, WAVES = kBlock / 64;
    static_assert(NV == 32, "the halving exchange below leaves accumulator j in lanes 2 j and 2 j + 1 of a 64-lane wavefront");
    __shared__ uint32_t part[WAVES][NV];
    __shared__ uint32_t part_hit[WAVES][Q];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t q0 = (uint64_t)blockIdx.x * Q;
    uint32_t u[Q];
    bool live[Q];
#pragma unroll
    for (uint32_t q = 0; q < Q; q++) {
        u[q] = q0 + q < n_seqs ? num_unique[q0 + q] : 0u;
        live[q] = u[q] != 0;
    }
    uint32_t grouped = 0;                                    // thread q < Q: the query's counts summed over the passes
    uint32_t hit_all = 0;                                    // thread q < Q: samples_hit (first pass)
    for (uint32_t g0 = 0; g0 < n_groups; g0 += GB) {
        uint32_t acc[NV], hit[Q];
#pragma unroll
        for (uint32_t i = 0; i < NV; i++) acc[i] = 0u;
#pragma unroll
        for (uint32_t q = 0; q < Q; q++) hit[q] = 0u;
#pragma unroll 1
        for (uint32_t w = threadIdx.x; w < wv; w += kBlock) {
            uint64_t m[GB], x[Q];
#pragma unroll
            for (uint32_t g = 0; g < GB; g++) m[g] = g0 + g < n_groups ? masks[(uint64_t)(g0 + g) * wv + w] : 0ull;
#pragma unroll
            for (uint32_t q = 0; q < Q; q++) x[q] = live[q] ? bitmaps[(q0 + q) * bm_stride + w] : 0ull;
#pragma unroll
            for (uint32_t q = 0; q < Q; q++)
#pragma unroll
                for (uint32_t g = 0; g < GB; g++) acc[q * GB + g] += (uint32_t)__popcll(x[q] & m[g]);
            if (g0 == 0) {
                const uint64_t vm = valid_mask(w, n_cols);
#pragma unroll
                for (uint32_t q = 0; q < Q; q++) hit[q] += (uint32_t)__popcll(x[q] & vm);
            }
        }
        group_halve<NV / 2>(acc, lane);
        acc[0] += __shfl_xor(acc[0], 1);
        if ((lane & 1u) == 0) part[wave][lane >> 1] = acc[0];
        if (g0 == 0) {
#pragma unroll
            for (uint32_t q = 0; q < Q; q++) {
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) hit[q] += __shfl_xor(hit[q], d);
                if (lane == 0) part_hit[wave][q] = hit[q];
            }
        }
        __syncthreads();
        if (threadIdx.x < NV) {
            const uint32_t q = threadIdx.x / GB, g = threadIdx.x % GB;
            uint32_t sum = 0;
#pragma unroll
            for (uint32_t i = 0; i < WAVES; i++) sum += part[i][threadIdx.x];
            if (q0 + q < n_seqs && g0 + g < n_groups) counts[(q0 + q) * n_groups + g0 + g] = sum;
        }
        if (threadIdx.x < Q) {
            for (uint32_t i = 0; i < WAVES; i++) {
                for (uint32_t g = 0; g < GB; g++) grouped += part[i][threadIdx.x * GB + g];
                if (g0 == 0) hit_all += part_hit[i][threadIdx.x];
            }
        }
        __syncthreads();
    }
    if (threadIdx.x < Q && q0 + threadIdx.x < n_seqs) {
        const uint32_t uq = num_unique[q0 + threadIdx.x];
        const double mkd = ceil((double)uq * threshold);          // min_kmers as K1 computes it
        const uint32_t mk = mkd > 0.0 ? (uint32_t)mkd : 0u;
        info[q0 + threadIdx.x] = make_uint4(uq, uq ? mk : 0u, hit_all, grouped);
    }
}

// ------------------------------------------------------------------------------ panel genotyping: every sample's call per variant
// The segmented OR over the result vectors a run made with BIGSI_RUN_SKIP_COMPACT left behind (include/bigsi_hip_genotype.h has the
// definition): the probes of one allele fold into one bit plane, planes[2 v + a][wv]; the calls come from two planes by AND, AND-NOT
// and popcount.  No work per hit: a ref probe that hits every column costs what one that hits none costs.
//
// k_allele_or (launch shape: plan_genotype): thread = result word w -- consecutive threads take consecutive words, coalesced 8-byte
//   loads, never w >= wv: the pad word of wv_pad is not read -- and a workgroup owns kBlock words and the probes [q0, q1) of one tile.
//   A thread walks the tile with (current allele, accumulated word) in registers, kGenotypeLoads loads in flight; allele_of and
//   num_unique of a probe are uniform, and a probe without k-mers or without an allele is skipped in a uniform branch before its word
//   is loaded.  valid_mask is applied before the OR.  When the allele changes, or the tile ends, the thread issues ONE 64-bit atomicOr
//   into planes[allele][w], and only if the word is non-zero: probes grouped by allele cost one atomic per allele, tile and word; any
//   other order costs more atomics and gives the same planes -- OR is idempotent and order-free, so chunks on two streams may meet in
//   one plane word.  Thread i of the workgroup that owns word 0 adds probe q0 + i into used[allele].  28 VGPRs, 34 SGPRs, no scratch, no spill.
// k_genotype_variants: one wavefront per variant.  The lanes sweep the words of both planes under sel[w] (columns & valid_mask, built
//   once at create), popcount r & ~a, r & a and a & ~r, and the wavefront reduces; one uint4 store per variant, missing = the selected
//   columns minus the other three; no atomic.  It leaves the planes masked (idempotent).  20 VGPRs, no scratch.
// k_genotype_samples: a wavefront owns word w, lane l the column 64 w + l at bit bit_of_col(l); a loop over all variants with
//   wave-uniform loads of the two (masked) words, four variants in flight; one plain uint2 store {carried, called} per column, the
//   ones behind num_cols included (they are zero: the planes are masked).  No atomic and nothing to zero.  11 VGPRs, no scratch.
__global__ __launch_bounds__(kBlock) void k_allele_or(
    const uint64_t *__restrict__ bitmaps, uint64_t bm_stride, uint32_t wv, uint64_t n_cols, uint32_t n_seqs,
    const uint32_t *__restrict__ num_unique, const uint32_t *__restrict__ allele_of, uint32_t word_blocks,
    unsigned long long *__restrict__ planes, uint32_t *__restrict__ used)
{
    const uint32_t t = blockIdx.x / word_blocks, wb = blockIdx.x - t * word_blocks;
    const uint32_t w = wb * kBlock + threadIdx.x;
    const uint32_t q0 = t * kGenotypeTile, q1 = n_seqs - q0 < kGenotypeTile ? n_seqs : q0 + kGenotypeTile;
    if (wb == 0 && threadIdx.x < q1 - q0) {
        const uint32_t al = allele_of[q0 + threadIdx.x];
        if (al != kGenotypeNone && num_unique[q0 + threadIdx.x] != 0) atomicAdd(&used[al], 1u);
    }
    if (w >= wv) return;
    const uint64_t vm = valid_mask(w, n_cols);
    uint32_t cur = kGenotypeNone;
    uint64_t acc = 0;
    for (uint32_t q = q0; q < q1; q += kGenotypeLoads) {
        uint32_t al[kGenotypeLoads];
        uint64_t x[kGenotypeLoads];
#pragma unroll
        for (uint32_t j = 0; j < kGenotypeLoads; j++) {
            al[j] = q + j < q1 ? allele_of[q + j] : kGenotypeNone;
            if (al[j] != kGenotypeNone && num_unique[q + j] == 0) al[j] = kGenotypeNone;
            x[j] = al[j] != kGenotypeNone ? bitmaps[(uint64_t)(q + j) * bm_stride + w] : 0ull;
        }
#pragma unroll
        for (uint32_t j = 0; j < kGenotypeLoads; j++) {
            if (al[j] == kGenotypeNone) continue;                       // (uniform)
            if (al[j] != cur) {
                if (acc) atomicOr(&planes[(uint64_t)cur * wv + w], (unsigned long long)acc);
                cur = al[j];
                acc = 0;
            }
            acc |= x[j] & vm;
        }
    }
    if (acc) atomicOr(&planes[(uint64_t)cur * wv + w], (unsigned long long)acc);
}

__global__ __launch_bounds__(kBlock) void k_genotype_variants(uint64_t *__restrict__ planes, const uint64_t *__restrict__ sel, uint32_t wv,
                                                              uint32_t n_variants, uint32_t n_selected, uint4 *__restrict__ variant_counts)
{
    const uint32_t v = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (v >= n_variants) return;                                        // (uniform over the wavefront)
    uint64_t *ref = planes + (uint64_t)(2 * v) * wv, *alt = ref + wv;
    uint32_t hom_ref = 0, het = 0, hom_alt = 0;
    for (uint32_t w = lane; w < wv; w += 64) {
        const uint64_t s = sel[w], r = ref[w] & s, a = alt[w] & s;
        ref[w] = r;
        alt[w] = a;
        hom_ref += (uint32_t)__popcll(r & ~a);
        het += (uint32_t)__popcll(r & a);
        hom_alt += (uint32_t)__popcll(a & ~r);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        hom_ref += __shfl_xor(hom_ref, d);
        het += __shfl_xor(het, d);
        hom_alt += __shfl_xor(hom_alt, d);
    }
    if (lane == 0) variant_counts[v] = make_uint4(hom_ref, het, hom_alt, n_selected - hom_ref - het - hom_alt);
}

__global__ __launch_bounds__(kBlock) void k_genotype_samples(const uint64_t *__restrict__ planes, uint32_t wv, uint32_t n_variants,
                                                             uint2 *__restrict__ sample_counts)
{
    const uint32_t w = blockIdx.x * (kBlock / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    if (w >= wv) return;
    const uint32_t bit = bit_of_col(lane);
    uint32_t carried = 0, called = 0;
    for (uint32_t v = 0; v < n_variants; v += 4) {
        uint64_t r[4], a[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            r[j] = v + j < n_variants ? planes[(uint64_t)(2 * (v + j)) * wv + w] : 0ull;
            a[j] = v + j < n_variants ? planes[(uint64_t)(2 * (v + j) + 1) * wv + w] : 0ull;
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            carried += (uint32_t)((a[j] >> bit) & 1ull);
            called += (uint32_t)(((r[j] | a[j]) >> bit) & 1ull);
        }
    }
    sample_counts[(uint64_t)w * 64 + lane] = make_uint2(carried, called);
}

// ------------------------------------------------------------------------------ locus typing: each sample's best allele per locus
// The segmented max with argmax over the result vectors AND counters a run made with BIGSI_RUN_SKIP_COMPACT left behind
// (include/bigsi_hip_typing.h has the definition): per (locus, column) the largest typing_key of the locus's records that hit the
// column -- best[l][64 w + lane], 0: no hit --, the number of such records -- hits[l][..] -- and per locus its records with k-mers.
//
// k_locus_best (launch shape: plan_typing): k_tally_hits' shape.  A wavefront owns result word w -- lane l the column 64 w + l at bit
//   bit_of_col(l) -- and the records [q0, q1) of one tile.  Per record ONE wave-uniform 8-byte load of the word, kTypingLoads in
//   flight, ANDed with sel[w] (columns & valid_mask, built once at create: bits behind num_cols are never trusted, and only words
//   < wv are read).  A zero word is skipped in a uniform branch before anything else of the record is touched; otherwise locus_of,
//   num_unique and allele_of of the record are uniform loads (no locus or no k-mers: skipped), and a lane whose bit is set loads its
//   own counter (a predicated load; in sparse mode the counters of a word that holds a hit are valid; EXACT never reads one: c = u),
//   takes typing_key -- the 64-bit division runs only here, in plain C++ -- and keeps (current locus, best key, hit count) in
//   registers.  On a locus change or at the tile end a lane issues one 64-bit atomicMax and one 32-bit atomicAdd, each only when
//   non-zero: records grouped by locus cost one pair per locus, tile and column; any other order costs more atomics and gives the same
//   cells -- max and add of integers are order-free, so chunks on two streams may meet in one cell.  Thread i of the workgroup that
//   owns word 0 adds record q0 + i to records[locus].  No LDS, no scratch, no spill.
// k_locus_counts (one launch at fetch, no atomics): workgroups below loci_grid give a wavefront to each locus -- the lanes sweep its
//   row of cells, count best != 0, score == 2^32 - 1 and hits > 1, and reduce by shuffles; three stores per locus.  The workgroups
//   behind them give a wavefront to each result word, lane = column, and loop over the loci (coalesced 8-byte loads, four in flight);
//   one uint2 store {called, exact} per column, the ones behind num_cols included (they are zero: their cells never got a key).
template <typename CountT, bool EXACT>
__global__ __launch_bounds__(kBlock) void k_locus_best(
    const uint64_t *__restrict__ bitmaps, uint64_t bm_stride, uint32_t wv, uint32_t n_seqs, const uint32_t *__restrict__ num_unique,
    const CountT *__restrict__ counters, uint64_t counter_stride, const uint32_t *__restrict__ locus_of, const uint32_t *__restrict__ allele_of,
    const uint64_t *__restrict__ sel, uint32_t word_groups, unsigned long long *__restrict__ best, uint32_t *__restrict__ hits,
    uint32_t *__restrict__ records)
{
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const uint32_t t = blockIdx.x / word_groups, wg = blockIdx.x - t * word_groups, w = wg * (kBlock / 64) + wave;
    const uint32_t q0 = t * kTypingTile, q1 = n_seqs - q0 < kTypingTile ? n_seqs : q0 + kTypingTile;
    if (wg == 0 && threadIdx.x < q1 - q0) {
        const uint32_t l = locus_of[q0 + threadIdx.x];
        if (l != kTypingNone && num_unique[q0 + threadIdx.x] != 0) atomicAdd(&records[l], 1u);
    }
    if (w >= wv) return;
    const uint64_t sm = sel[w], row = (uint64_t)wv * 64, cell = (uint64_t)w * 64 + lane;
    const uint32_t bit = bit_of_col(lane);
    uint32_t cur = kTypingNone, n_hits = 0;
    unsigned long long key = 0;
    for (uint32_t q = q0; q < q1; q += kTypingLoads) {
        uint64_t x[kTypingLoads];
#pragma unroll
        for (uint32_t j = 0; j < kTypingLoads; j++) x[j] = q + j < q1 ? bitmaps[(uint64_t)(q + j) * bm_stride + w] & sm : 0ull;
#pragma unroll
        for (uint32_t j = 0; j < kTypingLoads; j++) {
            if (x[j] == 0) continue;                                    // (uniform)
            const uint32_t l = locus_of[q + j];
            if (l == kTypingNone) continue;
            const uint32_t u = num_unique[q + j];
            if (u == 0) continue;
            if (l != cur) {
                if (key) atomicMax(&best[(uint64_t)cur * row + cell], key);
                if (n_hits) atomicAdd(&hits[(uint64_t)cur * row + cell], n_hits);
                cur = l;
                key = 0;
                n_hits = 0;
            }
            if ((x[j] >> bit) & 1ull) {
                const uint32_t al = allele_of[q + j];
                const unsigned long long mine =
                    EXACT ? typing_key(1u, 1u, al) : typing_key((uint32_t)counters[(uint64_t)(q + j) * counter_stride + cell], u, al);
                key = mine > key ? mine : key;
                n_hits++;
            }
        }
    }
    if (key) atomicMax(&best[(uint64_t)cur * row + cell], key);
    if (n_hits) atomicAdd(&hits[(uint64_t)cur * row + cell], n_hits);
}

__global__ __launch_bounds__(kBlock) void k_locus_counts(const uint64_t *__restrict__ best, const uint32_t *__restrict__ hits, uint32_t wv, uint32_t n_loci,
                                                         uint32_t loci_grid, uint32_t *__restrict__ locus_counts, uint2 *__restrict__ sample_counts)
{
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63u;
    const uint64_t row = (uint64_t)wv * 64;
    if (blockIdx.x < loci_grid) {
        const uint32_t l = blockIdx.x * (kBlock / 64) + wave;
        if (l >= n_loci) return;                                        // (uniform over the wavefront)
        uint32_t called = 0, exact = 0, multiple = 0;
        for (uint64_t i = lane; i < row; i += 64) {
            const uint64_t b = best[(uint64_t)l * row + i];
            called += b != 0 ? 1u : 0u;
            exact += (b >> 32) == 0xFFFFFFFFull ? 1u : 0u;
            multiple += hits[(uint64_t)l * row + i] > 1u ? 1u : 0u;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            called += __shfl_xor(called, d);
            exact += __shfl_xor(exact, d);
            multiple += __shfl_xor(multiple, d);
        }
        if (lane < 3) locus_counts[(uint64_t)l * 3 + lane] = lane == 0 ? called : lane == 1 ? exact : multiple;
        return;
    }
    const uint32_t w = (blockIdx.x - loci_grid) * (kBlock / 64) + wave;
    if (w >= wv) return;
    const uint64_t cell = (uint64_t)w * 64 + lane;
    uint32_t called = 0, exact = 0;
    for (uint32_t l = 0; l < n_loci; l += 4) {
        uint64_t b[4];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) b[j] = l + j < n_loci ? best[(uint64_t)(l + j) * row + cell] : 0ull;
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            called += b[j] != 0 ? 1u : 0u;
            exact += (b[j] >> 32) == 0xFFFFFFFFull ? 1u : 0u;
        }
    }
    sample_counts[cell] = make_uint2(called, exact);
}

}   // namespace bigsi
