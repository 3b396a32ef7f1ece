// bigsi_kmercount.hip -- the exact k-mer counter of libbigsi_hip.so (include/bigsi_hip_kmercount.h): host entry points and, through
// bigsi_kmercount_kernels.hpp, its kernels.  A translation unit of its own: nothing here is reached from a search, and the code object
// of the search kernels stays what it was.
#include "bigsi_internal.hpp"

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "bigsi_kmercount_kernels.hpp"

using namespace bigsi;

// ------------------------------------------------------------------------------ exact k-mer counter
// include/bigsi_hip_kmercount.h; k_count_kmers + k_kmer_table_{rehash,spectrum,bloom,fetch}; every decision about a call -- its
// positions, its refusal, its staging chunks, the table's size before a chunk -- is plan_kmer_count_add's and plan_kmer_table's
// (bigsi_launch.hpp).  A counter has a stream of its own and no index.  Per chunk: the pieces are copied behind one another into pinned
// memory, a separator byte behind each, uploaded, counted, and the four statistics words come back -- the host knows `distinct` before
// it sizes the table for the next chunk.  d_words: the statistics (kKmerStat*), the fetch cursor, the 256 spectrum bins.
struct bigsi_hip_kmer_counter {
    int device = 0;
    uint32_t k = 0;
    hipStream_t stream = nullptr;
    unsigned long long *d_keys = nullptr;
    uint32_t *d_counts = nullptr;
    uint64_t slots = 0;
    unsigned long long *d_words = nullptr;
    DevBuf stage;
    void *pin = nullptr;
    size_t pin_cap = 0;
    uint64_t counted = 0, skipped = 0, distinct = 0, invalid_starts = 0;
    uint64_t expected = 0, chunk_bytes = kKmerChunkBytes, initial_slots = 0;
    bool unusable = false;          // an add failed half way: until reset
};
enum { kKmerWordCursor = 4, kKmerWordBins = 8, kKmerWords = kKmerWordBins + 256 };

static void kmer_table_free(bigsi_hip_kmer_counter *c)
{
    hipError_t e = hipSuccess;
    if (c->d_keys) e = hipFree(c->d_keys);
    if (c->d_counts) e = hipFree(c->d_counts);
    (void)e;
    c->d_keys = nullptr; c->d_counts = nullptr; c->slots = 0;
}

// an empty table of `slots` slots, queued on the counter's stream; BIGSI_ERR_NOMEM when the device has no room for it
static int kmer_table_alloc(bigsi_hip_kmer_counter *c, uint64_t slots, unsigned long long **keys, uint32_t **counts)
{
    *keys = nullptr; *counts = nullptr;
    hipError_t e = hipMalloc((void **)keys, slots * 8);
    if (e == hipSuccess) e = hipMalloc((void **)counts, slots * 4);
    if (e == hipSuccess) e = hipMemsetAsync(*keys, 0xFF, slots * 8, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(*counts, 0, slots * 4, c->stream);
    if (e != hipSuccess) {
        hipError_t e2 = hipSuccess;
        if (*keys) e2 = hipFree(*keys);
        if (*counts) e2 = hipFree(*counts);
        (void)e2; (void)hipGetLastError();
        *keys = nullptr; *counts = nullptr;
        return fail(e == hipErrorOutOfMemory ? BIGSI_ERR_NOMEM : BIGSI_ERR_HIP, "k-mer table of %llu slots: %s", (unsigned long long)slots, hipGetErrorString(e));
    }
    return BIGSI_OK;
}

static unsigned kmer_sweep_grid(uint64_t slots) { return (unsigned)std::min<uint64_t>(ceil_div(slots, kBlock), 256 * 8); }

// the statistics words, after everything queued so far
static int kmer_read_stats(bigsi_hip_kmer_counter *c, unsigned long long st[4])
{
    HIP_TRY(hipMemcpyAsync(st, c->d_words, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BIGSI_OK;
}

static int kmer_table_grow(bigsi_hip_kmer_counter *c, uint64_t slots)
{
    unsigned long long *keys = nullptr;
    uint32_t *counts = nullptr;
    TRY(kmer_table_alloc(c, slots, &keys, &counts));
    hipLaunchKernelGGL(k_kmer_table_rehash, dim3(kmer_sweep_grid(c->slots)), dim3(kBlock), 0, c->stream, c->d_keys, c->d_counts, c->slots, keys, counts, slots, c->d_words);
    unsigned long long st[4] = {0, 0, 0, 0};
    hipError_t e = hipGetLastError();
    int rc = e == hipSuccess ? kmer_read_stats(c, st) : fail(BIGSI_ERR_HIP, "k_kmer_table_rehash: %s", hipGetErrorString(e));
    if (rc == BIGSI_OK && st[kKmerStatError]) rc = fail(BIGSI_ERR_STATE, "internal: a key found no slot while the table grew to %llu slots", (unsigned long long)slots);
    if (rc != BIGSI_OK) { e = hipFree(keys); e = hipFree(counts); (void)e; return rc; }
    kmer_table_free(c);
    c->d_keys = keys; c->d_counts = counts; c->slots = slots;
    return BIGSI_OK;
}

// an empty counter with a table of `slots` slots
static int kmer_counter_clear(bigsi_hip_kmer_counter *c, uint64_t slots)
{
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->slots != slots) {
        // the old table goes first (a reset under memory pressure must not need both at once); without a table the counter is
        // unusable -- every call but reset and destroy answers BIGSI_ERR_STATE, and a later reset tries the allocation again
        kmer_table_free(c);
        c->unusable = true;
        unsigned long long *keys = nullptr;
        uint32_t *counts = nullptr;
        TRY(kmer_table_alloc(c, slots, &keys, &counts));
        c->d_keys = keys; c->d_counts = counts; c->slots = slots;
    } else {
        HIP_TRY(hipMemsetAsync(c->d_keys, 0xFF, slots * 8, c->stream));
        HIP_TRY(hipMemsetAsync(c->d_counts, 0, slots * 4, c->stream));
    }
    HIP_TRY(hipMemsetAsync(c->d_words, 0, kKmerWords * 8, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->counted = c->skipped = c->distinct = c->invalid_starts = 0;
    c->unusable = false;
    return BIGSI_OK;
}

static int kmer_counter_usable(const bigsi_hip_kmer_counter *c)
{
    if (!c) return fail(BIGSI_ERR_INVALID, "NULL counter");
    if (c->unusable)
        return fail(BIGSI_ERR_STATE, "a bigsi_hip_kmer_counter_add on this counter failed half way, or its table could not be allocated: bigsi_hip_kmer_counter_reset starts over");
    return BIGSI_OK;
}

extern "C" int bigsi_hip_kmer_counter_create(int device, uint32_t k, uint64_t expected_distinct, bigsi_hip_kmer_counter **out)
{
    if (!out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (k == 0 || k > BIGSI_KMERCOUNT_MAX_K) return fail(BIGSI_ERR_INVALID, "k must be in [1, %u], got %u", BIGSI_KMERCOUNT_MAX_K, k);
    HIP_TRY(hipSetDevice(device));
    bigsi_hip_kmer_counter *c = new (std::nothrow) bigsi_hip_kmer_counter();
    if (!c) return fail(BIGSI_ERR_NOMEM, "host allocation failed");
    c->device = device; c->k = k; c->expected = expected_distinct;
    c->initial_slots = kmer_initial_slots(expected_distinct, kKmerInitialSlots);
    int rc = BIGSI_OK;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void **)&c->d_words, kKmerWords * 8);
    if (e != hipSuccess) rc = fail(e == hipErrorOutOfMemory ? BIGSI_ERR_NOMEM : BIGSI_ERR_HIP, "bigsi_hip_kmer_counter_create: %s", hipGetErrorString(e));
    if (rc == BIGSI_OK) rc = kmer_counter_clear(c, c->initial_slots);
    if (rc != BIGSI_OK) { bigsi_hip_kmer_counter_destroy(c); return rc; }
    *out = c;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_kmer_counter_destroy(bigsi_hip_kmer_counter *c)
{
    if (!c) return BIGSI_OK;
    hipError_t e = hipSetDevice(c->device);
    if (c->stream) { e = hipStreamSynchronize(c->stream); e = hipStreamDestroy(c->stream); }
    kmer_table_free(c);
    if (c->d_words) e = hipFree(c->d_words);
    if (c->pin) e = hipHostFree(c->pin);
    (void)e;
    c->stage.release();
    delete c;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_kmer_counter_reset(bigsi_hip_kmer_counter *c)
{
    if (!c) return fail(BIGSI_ERR_INVALID, "NULL counter");
    HIP_TRY(hipSetDevice(c->device));
    return kmer_counter_clear(c, c->initial_slots);
}

extern "C" int bigsi_hip_kmer_counter_set_limits(bigsi_hip_kmer_counter *c, uint64_t chunk_bytes, uint64_t initial_slots)
{
    TRY(kmer_counter_usable(c));
    if (c->counted + c->skipped + c->distinct) return fail(BIGSI_ERR_STATE, "the counter holds k-mers: set the limits right after create or reset");
    if (chunk_bytes && chunk_bytes < kKmerMinChunkBytes) return fail(BIGSI_ERR_INVALID, "chunk_bytes must be 0 or at least %llu", (unsigned long long)kKmerMinChunkBytes);
    if (initial_slots && (initial_slots < kKmerMinSlots || (initial_slots & (initial_slots - 1)) || initial_slots > (1ull << 34)))
        return fail(BIGSI_ERR_INVALID, "initial_slots must be 0 or a power of two in [%llu, 2^34]", (unsigned long long)kKmerMinSlots);
    HIP_TRY(hipSetDevice(c->device));
    c->chunk_bytes = chunk_bytes ? chunk_bytes : kKmerChunkBytes;
    c->initial_slots = initial_slots ? initial_slots : kmer_initial_slots(c->expected, kKmerInitialSlots);
    return kmer_counter_clear(c, c->initial_slots);
}

// one chunk of an accepted call: table first, then stage, upload, count, read the statistics back
static int kmer_count_chunk(bigsi_hip_kmer_counter *c, const char *seqs, const uint64_t *offsets, const KmerChunk &ch)
{
    const KmerTablePlan tp = plan_kmer_table(c->slots, c->distinct, ch.positions, ch.staged);
    if (tp.grow) TRY(kmer_table_grow(c, tp.slots));
    if (tp.grid > 0x7FFFFFFFull) return fail(BIGSI_ERR_INVALID, "chunk too large for one launch (%llu workgroups)", (unsigned long long)tp.grid);
    if (ch.staged > c->pin_cap) {          // the pinned staging buffer grows to the largest chunk seen (nothing is in flight: every chunk ends in a wait)
        if (c->pin) { hipError_t e = hipHostFree(c->pin); (void)e; c->pin = nullptr; c->pin_cap = 0; }
        HIP_TRY(hipHostMalloc(&c->pin, ch.staged, hipHostMallocDefault));
        c->pin_cap = ch.staged;
    }
    TRY(c->stage.reserve(round_up(ch.staged, kKmerTile) + 64));          // (a tile's last loads reach up to 32 bytes behind it)
    const uint64_t at = kmer_stage_chunk(seqs, offsets, ch, (uint8_t *)c->pin);
    if (at != ch.staged) return fail(BIGSI_ERR_STATE, "internal: staged %llu bytes of a chunk planned at %llu", (unsigned long long)at, (unsigned long long)ch.staged);
    HIP_TRY(hipMemcpyAsync(c->stage.p, c->pin, ch.staged, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_count_kmers, dim3((unsigned)tp.grid), dim3(tp.block), 0, c->stream, c->stage.as<uint8_t>(), ch.staged, c->k, c->d_keys, c->d_counts, c->slots,
                       c->d_words);
    HIP_TRY(hipGetLastError());
    unsigned long long st[4];
    TRY(kmer_read_stats(c, st));
    if (st[kKmerStatError]) return fail(BIGSI_ERR_STATE, "internal: a k-mer found no slot in a table of %llu slots", (unsigned long long)c->slots);
    const uint64_t counted = st[kKmerStatCounted] - c->counted, invalid = st[kKmerStatInvalid] - c->invalid_starts;
    if (counted + invalid != ch.staged || counted > ch.positions)          // every staged byte is one window start, valid or not
        return fail(BIGSI_ERR_STATE, "internal: %llu windows counted and %llu invalid over %llu staged bytes (%llu positions)", (unsigned long long)counted,
                    (unsigned long long)invalid, (unsigned long long)ch.staged, (unsigned long long)ch.positions);
    c->counted = st[kKmerStatCounted];
    c->invalid_starts = st[kKmerStatInvalid];
    c->skipped += ch.positions - counted;
    c->distinct = st[kKmerStatDistinct];
    return BIGSI_OK;
}

extern "C" int bigsi_hip_kmer_counter_add(bigsi_hip_kmer_counter *c, const char *seqs, const uint64_t *offsets, uint64_t n_seqs)
{
    TRY(kmer_counter_usable(c));
    if (n_seqs == 0) return BIGSI_OK;
    if (!offsets) return fail(BIGSI_ERR_INVALID, "NULL argument");
    // The order below -- plan from the offsets, refuse, and only then stage -- is what keeps a refused call from reading a byte behind
    // `seqs`.  tests/c_host/kmercount_plan_host.cpp (kc_host_add) restates it and runs it under AddressSanitizer over a nine-byte
    // buffer with the refused offsets: keep the two in step.
    KmerAddPlan plan;
    try {
        plan = plan_kmer_count_add(c->k, offsets, n_seqs, c->counted + c->skipped, c->chunk_bytes);
    } catch (const std::bad_alloc &) {          // (the chunk list of a very large call under a very small chunk limit)
        return fail(BIGSI_ERR_NOMEM, "host allocation failed while cutting the call into chunks: nothing of it was counted");
    }
    if (plan.refusal == KmerAddPlan::kNotMonotone) return fail(BIGSI_ERR_INVALID, "offsets must be non-decreasing (sequence %llu)", (unsigned long long)plan.bad_seq);
    if (offsets[n_seqs] - offsets[0] && !seqs) return fail(BIGSI_ERR_INVALID, "seqs is NULL");
    if (plan.refusal == KmerAddPlan::kLifetime)
        return fail(BIGSI_ERR_RANGE, "%llu more positions behind %llu: a k-mer counter takes at most 2^32 - 1 in its lifetime", (unsigned long long)plan.positions,
                    (unsigned long long)(c->counted + c->skipped));
    HIP_TRY(hipSetDevice(c->device));
    for (const KmerChunk &ch : plan.chunks) {
        if (ch.positions == 0) continue;          // nothing but pieces shorter than k
        const int rc = kmer_count_chunk(c, seqs, offsets, ch);
        if (rc != BIGSI_OK) {
            c->unusable = true;          // chunks before this one have been counted
            hipError_t e = hipStreamSynchronize(c->stream); (void)e;
            return rc;
        }
    }
    return BIGSI_OK;
}

extern "C" int bigsi_hip_kmer_counter_info(bigsi_hip_kmer_counter *c, uint64_t out[4])
{
    if (!c || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(kmer_counter_usable(c));
    out[0] = c->counted; out[1] = c->skipped; out[2] = c->distinct; out[3] = c->slots;
    return BIGSI_OK;
}

extern "C" int bigsi_hip_kmer_counter_spectrum(bigsi_hip_kmer_counter *c, uint64_t out[256])
{
    if (!c || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(kmer_counter_usable(c));
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long *bins = c->d_words + kKmerWordBins;
    HIP_TRY(hipMemsetAsync(bins, 0, 256 * 8, c->stream));
    hipLaunchKernelGGL(k_kmer_table_spectrum, dim3(kmer_sweep_grid(c->slots)), dim3(kBlock), 0, c->stream, c->d_keys, c->d_counts, c->slots, bins);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, bins, 256 * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return BIGSI_OK;
}

extern "C" int bigsi_hip_kmer_counter_fetch(bigsi_hip_kmer_counter *c, uint64_t *keys, uint32_t *counts, uint64_t capacity, uint64_t *n)
{
    if (!c || !n) return fail(BIGSI_ERR_INVALID, "NULL argument");
    TRY(kmer_counter_usable(c));
    *n = c->distinct;
    if (capacity < *n) return fail(BIGSI_ERR_CAPACITY, "the table holds %llu k-mers, the buffers %llu", (unsigned long long)*n, (unsigned long long)capacity);
    if (*n == 0) return BIGSI_OK;
    if (!keys || !counts) return fail(BIGSI_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t u = c->distinct;
    std::vector<unsigned long long> hk;
    std::vector<uint32_t> hc;
    std::vector<uint64_t> order;
    try {
        hk.resize(u); hc.resize(u); order.resize(u);
    } catch (const std::bad_alloc &) {
        return fail(BIGSI_ERR_NOMEM, "host allocation failed (%llu entries to sort)", (unsigned long long)u);
    }
    DevBuf dk, dc;
    unsigned long long cursor = 0;
    int rc = dk.reserve(u * 8);
    if (rc == BIGSI_OK) rc = dc.reserve(u * 4);
    if (rc == BIGSI_OK) {
        hipError_t e = hipMemsetAsync(c->d_words + kKmerWordCursor, 0, 8, c->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_kmer_table_fetch, dim3(kmer_sweep_grid(c->slots)), dim3(kBlock), 0, c->stream, c->d_keys, c->d_counts, c->slots,
                               dk.as<unsigned long long>(), dc.as<uint32_t>(), u, c->d_words + kKmerWordCursor);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(hk.data(), dk.p, u * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(hc.data(), dc.p, u * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&cursor, c->d_words + kKmerWordCursor, 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(BIGSI_ERR_HIP, "bigsi_hip_kmer_counter_fetch: %s", hipGetErrorString(e));
    }
    dk.release(); dc.release();
    if (rc != BIGSI_OK) return rc;
    if (cursor != u) return fail(BIGSI_ERR_STATE, "internal: the table holds %llu live slots, the counter %llu distinct keys", cursor, (unsigned long long)u);
    for (uint64_t i = 0; i < u; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return hk[a] < hk[b]; });
    for (uint64_t i = 0; i < u; i++) { keys[i] = hk[order[i]]; counts[i] = hc[order[i]]; }
    return BIGSI_OK;
}

extern "C" int bigsi_hip_kmer_counter_bloom(bigsi_hip_kmer_counter *c, uint64_t m, uint32_t h, uint32_t min_count, uint8_t *out)
{
    if (!c || !out) return fail(BIGSI_ERR_INVALID, "NULL argument");
    if (m == 0 || h == 0) return fail(BIGSI_ERR_INVALID, "m and h must be > 0");
    if (min_count == 0) return fail(BIGSI_ERR_INVALID, "min_count must be >= 1");
    TRY(kmer_counter_usable(c));
    HIP_TRY(hipSetDevice(c->device));
    const uint64_t nwords = ceil_div(m, 32), nb = ceil_div(m, 8);
    DevBuf bits;
    TRY(bits.reserve(nwords * 4));
    hipError_t e = hipMemsetAsync(bits.p, 0, nwords * 4, c->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_kmer_table_bloom, dim3(kmer_sweep_grid(c->slots)), dim3(kBlock), 0, c->stream, c->d_keys, c->d_counts, c->slots, c->k, min_count,
                           bits.as<uint32_t>(), m, h);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, bits.p, nb, hipMemcpyDeviceToHost, c->stream);   // little-endian words == byte order
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    bits.release();
    if (e != hipSuccess) return fail(BIGSI_ERR_HIP, "bigsi_hip_kmer_counter_bloom: %s", hipGetErrorString(e));
    return BIGSI_OK;
}
