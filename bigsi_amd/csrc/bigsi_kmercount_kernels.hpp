// bigsi_kmercount_kernels.hpp -- CDNA4 (gfx950) device code of the exact k-mer counter (include/bigsi_hip_kmercount.h):
// k_count_kmers and k_kmer_table_rehash / spectrum / bloom / fetch.  Compiled by bigsi_kmercount.hip into a code object of its own,
// so that the code object of the query and build kernels (bigsi_kernels.hpp, bigsi_hip.hip) does not change when this file does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bigsi_launch.hpp"      // kBlock, kKmerTile, kKmerLane: shared with the host's planner
#include "bigsi_device.hpp"      // mix64, murmur3_32, row_of_hash

namespace bigsi {

// ------------------------------------------------------------------------------ exact k-mer counter (include/bigsi_hip_kmercount.h)
// The table: open addressing in HBM, uint64 keys[slots] (kKmerEmpty = ~0: no canonical key for k <= 32) and uint32 counts[slots],
// slots a power of two.  The slot of a key comes from mix64 of it -- never its low bits, which are the last bases.  An insert is a
// 64-bit compare-and-swap on the key, then an atomic add on the count; linear probing.  A key never leaves its slot and a slot never
// changes its key, so a stale read can only show an empty slot that is no longer empty -- which the compare-and-swap then answers.
// The probe loop is bounded by the slot count: a key that finds no slot reports it (false) instead of spinning; the host keeps the
// table at most half full (plan_kmer_table), so this is a defect's exit, not a route.
constexpr uint64_t kKmerEmpty = ~0ull;
enum { kKmerStatCounted = 0, kKmerStatInvalid = 1, kKmerStatDistinct = 2, kKmerStatError = 3 };

__device__ __forceinline__ bool kmer_table_add(unsigned long long *__restrict__ keys, uint32_t *__restrict__ counts, uint64_t slots, uint64_t key, uint32_t n, bool *is_new)
{
    const uint64_t mask = slots - 1;
    uint64_t slot = mix64(key) & mask;
    *is_new = false;
    for (uint64_t probe = 0; probe < slots; probe++, slot = (slot + 1) & mask) {
        unsigned long long cur = keys[slot];
        if (cur == kKmerEmpty) {
            cur = atomicCAS(&keys[slot], (unsigned long long)kKmerEmpty, (unsigned long long)key);
            if (cur == kKmerEmpty) { *is_new = true; cur = key; }
        }
        if (cur == key) {
            atomicAdd(&counts[slot], n);
            return true;
        }
    }
    return false;
}

// k_count_kmers (launch shape: plan_kmer_table's grid).  The staged stream is a chunk's pieces behind one another, one separator byte
// (no base) behind each, so a window that spans two reads holds an invalid byte like one that holds an N.  A workgroup owns the
// kKmerTile window starts [t0, t0 + kKmerTile) and needs the bytes up to k - 1 <= 31 behind them: kBlock + 2 words of 16 bases.  Every
// thread loads 16 bytes (aligned: t0 is a multiple of the tile and the buffer the allocator's; the buffer is padded behind the last
// tile) and writes one word of 2-bit codes (A 0, C 1, G 2, T 3, acgt folded; the first base in the highest bits) and its 16-bit
// invalid mask into LDS; a byte at or behind `staged` is invalid whatever it holds.  Then a thread owns kKmerLane consecutive starts:
// from three code words it forms the first window's forward word by a funnel shift, its reverse complement by a bit reversal, and
// rolls both one base at a time -- nothing per position depends on k.  The key is the smaller of the two.
// Contention: at step j the lanes of a wavefront hold the windows 16 l + j.  Neighbouring lanes with equal keys (a homopolymer, and
// every repeat whose period divides 16) are combined before the atomic: the first lane of a run adds the run's length.  New keys,
// counted windows and invalid window starts are summed per wavefront (ballots) and leave as one atomic each per wavefront.
__global__ __launch_bounds__(kBlock) void k_count_kmers(
    const uint8_t *__restrict__ stream, uint64_t staged, uint32_t k, unsigned long long *__restrict__ keys, uint32_t *__restrict__ counts, uint64_t slots,
    unsigned long long *__restrict__ stats)
{
    __shared__ uint32_t s_code[kBlock + 2], s_inv[kBlock + 2];
    const uint64_t t0 = (uint64_t)blockIdx.x * kKmerTile;
    for (uint32_t w = threadIdx.x; w < kBlock + 2; w += kBlock) {
        const uint64_t at = t0 + (uint64_t)w * kKmerLane;
        uint32_t code = 0, inv = 0xFFFFu;
        if (at < staged) {
            const uint4 raw = *reinterpret_cast<const uint4 *>(stream + at);
            const uint32_t r[4] = {raw.x, raw.y, raw.z, raw.w};
            inv = 0;
#pragma unroll
            for (uint32_t i = 0; i < kKmerLane; i++) {
                const uint32_t up = ((r[i >> 2] >> (8 * (i & 3))) & 0xFFu) & 0xDFu;          // a-z onto A-Z; nothing else lands on a base
                const bool base = (up == 'A') | (up == 'C') | (up == 'G') | (up == 'T');
                uint32_t c = (up >> 1) & 3u;                                                // A 0, C 1, T 2, G 3
                c ^= c >> 1;                                                                // A 0, C 1, G 2, T 3
                code |= c << (2 * (kKmerLane - 1 - i));
                inv |= (uint32_t)(!base || at + i >= staged) << i;
            }
        }
        s_code[w] = code;
        s_inv[w] = inv;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, t = threadIdx.x;
    const uint64_t w01 = ((uint64_t)s_code[t] << 32) | s_code[t + 1];          // bases 0..31 behind the thread's first start
    const uint32_t w2 = s_code[t + 2];                                          // bases 32..47
    const uint64_t inv48 = (uint64_t)s_inv[t] | ((uint64_t)s_inv[t + 1] << 16) | ((uint64_t)s_inv[t + 2] << 32);
    const uint64_t kmask = k == 32 ? ~0ull : (1ull << (2 * k)) - 1, wmask = (1ull << k) - 1;          // (k <= 32: wmask fits)
    uint64_t fwd = w01 >> (2 * (32 - k));
    // reverse complement: reverse the 2-bit groups of the word, complement, down to the low 2k bits
    uint64_t rev = __builtin_bitreverse64(fwd);
    rev = ((rev & 0xAAAAAAAAAAAAAAAAull) >> 1) | ((rev & 0x5555555555555555ull) << 1);
    uint64_t rc = (~rev) >> (2 * (32 - k));
    const uint64_t p0 = t0 + (uint64_t)t * kKmerLane;
    uint32_t n_counted = 0, n_invalid = 0, n_new = 0, failed = 0;          // wavefront sums, the same in every lane
#pragma unroll 1
    for (uint32_t j = 0; j < kKmerLane; j++) {
        if (j) {
            const uint32_t i = k - 1 + j;                                  // the base that enters: 1 <= i <= 46
            const uint32_t c = i < 32 ? (uint32_t)(w01 >> (2 * (31 - i))) & 3u : (w2 >> (2 * (47 - i))) & 3u;
            fwd = ((fwd << 2) | c) & kmask;
            rc = (rc >> 2) | ((uint64_t)(3u - c) << (2 * (k - 1)));
        }
        const bool start = p0 + j < staged;
        const bool valid = start && ((inv48 >> j) & wmask) == 0;
        const uint64_t key = fwd < rc ? fwd : rc;
        const uint64_t vmask = __ballot((int)valid);
        n_counted += (uint32_t)__popcll(vmask);
        n_invalid += (uint32_t)__popcll(__ballot((int)(start && !valid)));
        if (vmask == 0) continue;                                          // (uniform)
        const uint32_t prev_lo = (uint32_t)__shfl_up((int)(uint32_t)key, 1), prev_hi = (uint32_t)__shfl_up((int)(uint32_t)(key >> 32), 1);
        const bool joins = lane > 0 && ((vmask >> (lane - 1)) & 1ull) && (((uint64_t)prev_hi << 32) | prev_lo) == key;      // continues the lane below's run
        const bool head = valid && !joins;
        const uint64_t ends = __ballot((int)(head || !valid));             // lanes at which no run continues
        bool is_new = false, ok = true;
        if (head) {
            const uint64_t above = lane == 63 ? 0ull : ends >> (lane + 1);
            const uint32_t run = above ? (uint32_t)__ffsll((long long)above) : 64u - lane;
            ok = kmer_table_add(keys, counts, slots, key, run, &is_new);
        }
        n_new += (uint32_t)__popcll(__ballot((int)is_new));
        failed |= __ballot((int)!ok) ? 1u : 0u;
    }
    if (lane == 0) {
        if (n_counted) atomicAdd(&stats[kKmerStatCounted], (unsigned long long)n_counted);
        if (n_invalid) atomicAdd(&stats[kKmerStatInvalid], (unsigned long long)n_invalid);
        if (n_new) atomicAdd(&stats[kKmerStatDistinct], (unsigned long long)n_new);
        if (failed) atomicOr(&stats[kKmerStatError], 1ull);
    }
}

// k_kmer_table_rehash: every live slot of the old table into a new one of twice the size or more (the host zeroes it first and frees
// the old one afterwards).  Keys are distinct, so no insert meets its own key; the counts arrive by the same atomic add.
__global__ __launch_bounds__(kBlock) void k_kmer_table_rehash(
    const unsigned long long *__restrict__ old_keys, const uint32_t *__restrict__ old_counts, uint64_t old_slots,
    unsigned long long *__restrict__ keys, uint32_t *__restrict__ counts, uint64_t slots, unsigned long long *__restrict__ stats)
{
    bool failed = false;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < old_slots; i += (uint64_t)gridDim.x * kBlock) {
        const unsigned long long key = old_keys[i];
        if (key == kKmerEmpty) continue;
        bool is_new;
        failed |= !kmer_table_add(keys, counts, slots, key, old_counts[i], &is_new);
    }
    if (failed) atomicOr(&stats[kKmerStatError], 1ull);
}

// k_kmer_table_spectrum: out[min(count, 255)] += 1 per live slot.  An LDS histogram of 256 bins per workgroup (a workgroup sees fewer
// than 2^32 slots: the bins are uint32), then one 64-bit atomic per non-zero bin.
__global__ __launch_bounds__(kBlock) void k_kmer_table_spectrum(
    const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ counts, uint64_t slots, unsigned long long *__restrict__ out)
{
    __shared__ uint32_t bins[256];
    static_assert(kBlock == 256, "a thread per bin");
    bins[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * kBlock) {
        if (keys[i] == kKmerEmpty) continue;
        const uint32_t c = counts[i];
        atomicAdd(&bins[c < 255u ? c : 255u], 1u);
    }
    __syncthreads();
    if (bins[threadIdx.x]) atomicAdd(&out[threadIdx.x], (unsigned long long)bins[threadIdx.x]);
}

// the bases of a key as the bytes of its upper-case string: what murmur3_32 hashes for the filter (k_bloom hashes the same bytes)
struct KeyView {
    uint64_t key;
    uint32_t k;
    __device__ __forceinline__ uint8_t operator[](uint32_t j) const
    {
        return (uint8_t)(0x54474341u >> (8u * (uint32_t)((key >> (2 * (k - 1 - j))) & 3ull)));          // "ACGT"
    }
};

// k_kmer_table_bloom: the filter of the keys with count >= min_count, in k_bloom's byte and bit order (the keys are canonical: hashed
// as they are, BIGSI_BLOOM_RAW or not).
__global__ __launch_bounds__(kBlock) void k_kmer_table_bloom(
    const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ counts, uint64_t slots, uint32_t k, uint32_t min_count,
    uint32_t *__restrict__ bloom_words, uint64_t m, uint32_t h)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * kBlock) {
        const unsigned long long key = keys[i];
        if (key == kKmerEmpty || counts[i] < min_count) continue;
        const KeyView v{key, k};
        for (uint32_t sd = 0; sd < h; sd++) {
            const uint64_t r = row_of_hash(murmur3_32(v, sd), m);
            atomicOr(&bloom_words[r >> 5], 1u << (8u * (uint32_t)((r >> 3) & 3u) + 7u - (uint32_t)(r & 7u)));
        }
    }
}

// k_kmer_table_fetch: the live slots compacted into out_keys / out_counts (capacity: the table's distinct keys), in no order -- one
// aggregated atomic per wavefront and step hands out the places; the host sorts.
__global__ __launch_bounds__(kBlock) void k_kmer_table_fetch(
    const unsigned long long *__restrict__ keys, const uint32_t *__restrict__ counts, uint64_t slots,
    unsigned long long *__restrict__ out_keys, uint32_t *__restrict__ out_counts, uint64_t capacity, unsigned long long *__restrict__ cursor)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t step = (uint64_t)gridDim.x * kBlock, rounds = (slots + step - 1) / step;
    for (uint64_t r = 0; r < rounds; r++) {                                // (uniform trip count: every lane reaches the ballot)
        const uint64_t i = r * step + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
        const unsigned long long key = i < slots ? keys[i] : kKmerEmpty;
        const bool live = key != kKmerEmpty;
        const uint64_t lives = __ballot((int)live);
        if (lives == 0) continue;
        const uint32_t leader = (uint32_t)__ffsll((long long)lives) - 1u;
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd(cursor, (unsigned long long)__popcll(lives));
        const uint32_t b_lo = (uint32_t)__shfl((int)(uint32_t)base, (int)leader), b_hi = (uint32_t)__shfl((int)(uint32_t)(base >> 32), (int)leader);
        const uint64_t at = (((uint64_t)b_hi << 32) | b_lo) + (uint64_t)__popcll(lives & ((1ull << lane) - 1));
        if (live && at < capacity) { out_keys[at] = key; out_counts[at] = counts[i]; }
    }
}

}   // namespace bigsi
