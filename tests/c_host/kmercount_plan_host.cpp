// CPU pin of the k-mer counter's host-only planners (bigsi_amd/csrc/bigsi_launch.hpp): plan_kmer_count_add -- a call's positions, its
// refusal and its staging chunks, from the offsets alone --, kmer_stage_chunk, plan_kmer_table and kmer_initial_slots, compiled here
// as plain host C++.  Built two ways by tests/test_kmercount_plan_host.py: as a shared object whose functions it checks against the
// Python restatement (tests/kmercount_ref.py), and -- with KMERCOUNT_PLAN_MAIN -- as a stand-alone program under AddressSanitizer and
// UndefinedBehaviorSanitizer that hands kc_host_add, the host half of bigsi_hip_kmer_counter_add, buffers it must not overrun.
// Test infrastructure only: nothing in the product loads this file.
#include "../../bigsi_amd/csrc/bigsi_launch.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

extern "C" {

// out[]: kKmerCountLifetime, kKmerChunkBytes, kKmerMinChunkBytes, kKmerInitialSlots, kKmerMinSlots, kKmerTile, kKmerLane, kBlock
void kc_constants(uint64_t *out)
{
    const uint64_t v[8] = {bigsi::kKmerCountLifetime, bigsi::kKmerChunkBytes, bigsi::kKmerMinChunkBytes, bigsi::kKmerInitialSlots, bigsi::kKmerMinSlots,
                           bigsi::kKmerTile, bigsi::kKmerLane, (uint64_t)bigsi::kBlock};
    for (int i = 0; i < 8; i++) out[i] = v[i];
}

// head[]: refusal (0 none, 1 offsets decrease, 2 lifetime bound), bad_seq, positions; chunks[]: begin, end, seq0, seq1, positions,
// staged per chunk (at most `capacity` chunks are written); returns the number of chunks
uint64_t kc_plan_add(uint32_t k, const uint64_t *offsets, uint64_t n_seqs, uint64_t taken, uint64_t chunk_bytes, uint64_t *head, uint64_t *chunks, uint64_t capacity)
{
    const bigsi::KmerAddPlan p = bigsi::plan_kmer_count_add(k, offsets, n_seqs, taken, chunk_bytes);
    head[0] = (uint64_t)p.refusal; head[1] = p.bad_seq; head[2] = p.positions;
    for (size_t i = 0; i < p.chunks.size() && i < capacity; i++) {
        const bigsi::KmerChunk &c = p.chunks[i];
        const uint64_t v[6] = {c.begin, c.end, c.seq0, c.seq1, c.positions, c.staged};
        for (int j = 0; j < 6; j++) chunks[6 * i + j] = v[j];
    }
    return p.chunks.size();
}

// out[]: slots, grow, grid
void kc_plan_table(uint64_t slots_now, uint64_t distinct, uint64_t chunk_positions, uint64_t chunk_staged, uint64_t *out)
{
    const bigsi::KmerTablePlan p = bigsi::plan_kmer_table(slots_now, distinct, chunk_positions, chunk_staged);
    out[0] = p.slots; out[1] = p.grow ? 1 : 0; out[2] = p.grid;
}

uint64_t kc_initial_slots(uint64_t expected_distinct, uint64_t floor_slots) { return bigsi::kmer_initial_slots(expected_distinct, floor_slots); }

// The host half of bigsi_hip_kmer_counter_add, in its order: plan, refuse (-1 offsets decrease, -4 lifetime bound) before a byte
// behind seqs is touched, then stage every chunk -- here into a heap buffer of exactly the planned size.  out[0]: the call's
// positions; out[1]: the window starts of the staged streams that hold no separator (for input without NUL bytes: the same number).
int kc_host_add(uint32_t k, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint64_t taken, uint64_t chunk_bytes, uint64_t *out)
{
    out[0] = out[1] = 0;
    const bigsi::KmerAddPlan p = bigsi::plan_kmer_count_add(k, offsets, n_seqs, taken, chunk_bytes);
    if (p.refusal == bigsi::KmerAddPlan::kNotMonotone) return -1;
    if (p.refusal == bigsi::KmerAddPlan::kLifetime) return -4;
    out[0] = p.positions;
    for (const bigsi::KmerChunk &c : p.chunks) {
        uint8_t *buf = (uint8_t *)malloc(c.staged ? c.staged : 1);
        if (!buf) return -3;
        const uint64_t at = bigsi::kmer_stage_chunk(seqs, offsets, c, buf);
        uint64_t windows = 0, run = 0;          // run: bytes since the last separator
        for (uint64_t i = 0; i < at; i++) {
            run = buf[i] ? run + 1 : 0;
            windows += run >= k;
        }
        free(buf);
        if (at != c.staged || windows != c.positions) return -6;
        out[1] += windows;
    }
    return 0;
}

}

#ifdef KMERCOUNT_PLAN_MAIN
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("kmercount planner: line %d: %s\n", __LINE__, #cond);  \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main()
{
    uint64_t out[2];
    // refused calls over a nine-byte heap buffer: offsets that claim 2^32 + 4 bytes at k = 5 are 2^32 windows, one more than a counter
    // takes; were a byte behind them read, the sanitizer would end the program here
    {
        char *nine = (char *)malloc(9);
        CHECK(nine);
        memcpy(nine, "ACGTACGTA", 9);
        const uint64_t over[2] = {0, (1ull << 32) + 4};
        CHECK(kc_host_add(5, nine, over, 1, 0, 4096, out) == -4 && out[0] == 0 && out[1] == 0);
        const uint64_t one_over[2] = {0, (1ull << 32) + 3 - 5 + 1};          // 2^32 - 5 windows behind 5 taken: one too many
        CHECK(kc_host_add(5, nine, one_over, 1, 5, 4096, out) == -4);
        const uint64_t down[3] = {0, 9, 4};
        CHECK(kc_host_add(5, nine, down, 2, 0, 4096, out) == -1);
        const uint64_t honest[2] = {0, 9};
        CHECK(kc_host_add(5, nine, honest, 1, 0xFFFFFFFFull - 5, 64, out) == 0 && out[0] == 5 && out[1] == 5);          // the exact fit
        CHECK(kc_host_add(5, nine, honest, 1, 0xFFFFFFFFull - 4, 64, out) == -4);
        const uint64_t inner[3] = {2, 2, 9};                                  // offsets[0] > 0 and an empty read
        CHECK(kc_host_add(5, nine, inner, 2, 0, 64, out) == 0 && out[0] == 3 && out[1] == 3);
        free(nine);
    }
    // accepted calls over a buffer of exactly the bytes named: every chunk staged, no byte beyond read
    const uint32_t ks[3] = {5, 31, 32};
    const uint64_t limits[3] = {64, 100, 4096};
    for (uint32_t k : ks)
        for (uint64_t limit : limits) {
            const uint64_t lengths[] = {k - 1, k, k + 1, 0, 31, 32, 33, 63, 64, 65, 95 + k, 1023, 1024, 1025, 2 * limit + 3, 0, limit, limit + 1, limit + k - 1, 1};
            const size_t n = sizeof lengths / sizeof lengths[0];
            uint64_t off[n + 1], positions = 0;
            off[0] = 0;
            for (size_t i = 0; i < n; i++) { off[i + 1] = off[i] + lengths[i]; positions += lengths[i] >= k ? lengths[i] - k + 1 : 0; }
            char *buf = (char *)malloc(off[n]);
            CHECK(buf);
            for (uint64_t i = 0; i < off[n]; i++) buf[i] = "ACGT"[(i * 2654435761u >> 7) & 3];
            CHECK(kc_host_add(k, buf, off, n, 0, limit, out) == 0 && out[0] == positions && out[1] == positions);
            free(buf);
        }
    // the table rule
    uint64_t t[3];
    kc_plan_table(64, 0, 32, 33, t);
    CHECK(t[0] == 64 && t[1] == 0 && t[2] == 1);
    kc_plan_table(64, 1, 32, 4097, t);
    CHECK(t[0] == 128 && t[1] == 1 && t[2] == 2);
    kc_plan_table(0, 0xFFFFFFFFull, 0xFFFFFFFFull, 0, t);
    CHECK(t[0] == (1ull << 34) && t[2] == 0);
    CHECK(kc_initial_slots(0, 1 << 16) == (1 << 16) && kc_initial_slots(1 << 16, 1 << 16) == (1 << 17) && kc_initial_slots(~0ull, 64) == (1ull << 33));
    printf("kmercount planner: ok\n");
    return 0;
}
#endif
