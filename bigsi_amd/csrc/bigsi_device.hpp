// bigsi_device.hpp -- the small device helpers every kernel header shares: bit order of a row word, the reference's complement and
// canonical form, MurmurHash3_x86_32 over a view of a k-mer's bytes, the floor-mod row of a hash.  Included by bigsi_kernels.hpp (the
// query and build kernels) and bigsi_kmercount_kernels.hpp (the exact k-mer counter, a translation unit of its own).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bigsi {

// ------------------------------------------------------------------------------ small helpers
__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// bit position, inside the little-endian uint64 of a row, of column (8*byte + j)
__host__ __device__ __forceinline__ uint32_t bit_of_col(uint32_t c) { return ((c >> 3) & 7u) * 8u + 7u - (c & 7u); }

// column-order view of a word in row bit order: reverse the bits inside every byte
__device__ __forceinline__ uint64_t by_column(uint64_t x)
{
    const uint32_t lo = __builtin_bswap32(__builtin_bitreverse32((uint32_t)x)), hi = __builtin_bswap32(__builtin_bitreverse32((uint32_t)(x >> 32)));
    return ((uint64_t)hi << 32) | lo;
}

// mask of the valid column bits of word w for an index of n_cols columns (pad bits stay zero)
__host__ __device__ __forceinline__ uint64_t valid_mask(uint64_t w, uint64_t n_cols)
{
    uint64_t c0 = w * 64;
    if (c0 + 64 <= n_cols) return ~0ull;
    if (c0 >= n_cols) return 0ull;
    uint64_t mask = 0;
    for (int b = 0; b < 8; b++) {
        uint64_t cb = c0 + 8 * (uint64_t)b;
        uint64_t n = cb >= n_cols ? 0 : (n_cols - cb >= 8 ? 8 : n_cols - cb);
        mask |= (uint64_t)((0xFFu << (8 - n)) & 0xFFu) << (8 * b);
    }
    return mask;
}

// reverse_comp's per-base map (bigsi/utils/fncts.py:12,38-39): A<->T, C<->G, anything else unchanged
__device__ __forceinline__ uint8_t complement(uint8_t c)
{
    // branchless: 'A' ^ 'T' == 0x15 and 'C' ^ 'G' == 0x04 (a chain of ?: compiles to divergent exec-mask branches, and this
    // runs 2k times per k-mer)
    const uint32_t x = c;
    const uint32_t at = (uint32_t)(x == 'A') | (uint32_t)(x == 'T');
    const uint32_t cg = (uint32_t)(x == 'C') | (uint32_t)(x == 'G');
    return (uint8_t)(x ^ (at * 0x15u) ^ (cg * 0x04u));
}

// byte j of the canonical form of the k-mer at s[0..k): forward strand or reverse complement
struct KmerView {
    const char *s;
    uint32_t k;
    bool rc;
    __device__ __forceinline__ uint8_t operator[](uint32_t j) const
    {
        return rc ? complement((uint8_t)s[k - 1 - j]) : (uint8_t)s[j];
    }
};

// canonical (bigsi/utils/fncts.py:51-54): lexicographic min of k-mer and reverse complement -> use rc?
__device__ __forceinline__ bool use_revcomp(const char *s, uint32_t k)
{
    for (uint32_t j = 0; j < k; j++) {
        uint8_t f = (uint8_t)s[j], r = complement((uint8_t)s[k - 1 - j]);
        if (f != r) return r < f;
    }
    return false;
}

// mmh3.hash(kmer, seed) (bigsi/bloom/bloomfilter.py:6): MurmurHash3_x86_32, Austin Appleby's public-domain
// algorithm, over the k bytes of the view (KmerView: bytes of a sequence; KeyView: the bases of a packed k-mer counter key).
template <typename View>
__device__ __forceinline__ uint32_t murmur3_32(const View &v, uint32_t seed)
{
    const uint32_t c1 = 0xcc9e2d51u, c2 = 0x1b873593u;
    uint32_t h1 = seed;
    const uint32_t len = v.k, nblocks = len >> 2;
    for (uint32_t i = 0; i < nblocks; i++) {
        uint32_t k1 = (uint32_t)v[4 * i] | ((uint32_t)v[4 * i + 1] << 8) | ((uint32_t)v[4 * i + 2] << 16) |
                      ((uint32_t)v[4 * i + 3] << 24);
        k1 *= c1; k1 = rotl32(k1, 15); k1 *= c2;
        h1 ^= k1; h1 = rotl32(h1, 13); h1 = h1 * 5u + 0xe6546b64u;
    }
    uint32_t k1 = 0;
    const uint32_t t = nblocks * 4, rem = len & 3u;
    if (rem == 3) k1 ^= (uint32_t)v[t + 2] << 16;
    if (rem >= 2) k1 ^= (uint32_t)v[t + 1] << 8;
    if (rem >= 1) { k1 ^= (uint32_t)v[t]; k1 *= c1; k1 = rotl32(k1, 15); k1 *= c2; h1 ^= k1; }
    h1 ^= len;
    h1 ^= h1 >> 16; h1 *= 0x85ebca6bu; h1 ^= h1 >> 13; h1 *= 0xc2b2ae35u; h1 ^= h1 >> 16;
    return h1;
}

// _hash (bigsi/bloom/bloomfilter.py:5-6): signed 32-bit hash, Python floor-mod by m -> row in [0, m)
__device__ __forceinline__ uint64_t row_of_hash(uint32_t h, uint64_t m)
{
    const int32_t sh = (int32_t)h;
    const uint32_t mag = sh >= 0 ? (uint32_t)sh : 0u - (uint32_t)sh;      // |hash| <= 2^31 fits 32 bits
    if (m <= 0xFFFFFFFFull) {                                              // (wave-uniform) 32-bit division: ~4x cheaper than 64-bit
        const uint32_t a = mag % (uint32_t)m;
        return sh >= 0 || a == 0 ? (uint64_t)a : m - a;
    }
    const uint64_t a = (uint64_t)mag % m;
    return sh >= 0 || a == 0 ? a : m - a;
}

}   // namespace bigsi
