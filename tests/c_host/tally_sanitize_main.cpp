// A stand-alone program (its own main) that drives the host planners of the query-set tally (plan_tally, plan_tally_chunks,
// bigsi_amd/csrc/bigsi_launch.hpp) and the CPU twin's bigsi_cpu_search_tally (bigsi_amd/cpu/bigsi_cpu.cpp) over odd shapes, checks the
// planners' invariants and the twin against the twin's own per-sequence search, and is meant to be built with
// -fsanitize=address,undefined and run on the CPU: tests/test_tally_host.py compiles it together with bigsi_cpu.cpp and runs it.
// Nothing sanitized is loaded into Python.
// Test infrastructure only: nothing in the product loads this file.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../bigsi_amd/csrc/bigsi_launch.hpp"
#include "bigsi_cpu_tally.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            fprintf(stderr, "FAILED %s: ", #cond);        \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
            exit(1);                                      \
        }                                                 \
    } while (0)

// every chunk within the three bounds (or one sequence), the chunks covering [0, n) once and in order
static void chunk_shape(const std::vector<uint64_t> &lengths, uint32_t k, uint64_t wv_pad, uint32_t count_bytes)
{
    const uint64_t n = lengths.size();
    std::vector<uint64_t> off(n + 1, 0);
    for (uint64_t i = 0; i < n; i++) off[i + 1] = off[i] + lengths[i];
    const std::vector<uint64_t> cut = bigsi::plan_tally_chunks(off.data(), n, k, wv_pad, count_bytes);
    CHECK(!cut.empty() && cut.front() == 0 && cut.back() == n, "the cuts of %llu sequences do not span them", (unsigned long long)n);
    for (size_t c = 0; c + 1 < cut.size(); c++) {
        CHECK(cut[c] < cut[c + 1], "an empty chunk");
        const uint64_t seqs = cut[c + 1] - cut[c];
        uint64_t pos = 0;
        for (uint64_t s = cut[c]; s < cut[c + 1]; s++) pos += lengths[s] >= k ? lengths[s] - k + 1 : 0;
        CHECK(seqs <= bigsi::kTallyChunkSeqs, "a chunk of %llu sequences", (unsigned long long)seqs);
        CHECK(seqs == 1 || pos <= bigsi::kTallyChunkPositions, "a chunk of %llu positions", (unsigned long long)pos);
        CHECK(seqs == 1 || seqs * wv_pad * 64 * count_bytes <= bigsi::kTallyCounterBytes, "a chunk of %llu counter bytes", (unsigned long long)(seqs * wv_pad * 64 * count_bytes));
        CHECK(bigsi::tally_chunk_end(off.data(), n, cut[c], k, wv_pad, count_bytes) == cut[c + 1], "tally_chunk_end disagrees with the cuts");
    }
}

static void planners()
{
    for (uint64_t n : {1ull, 2ull, 127ull, 128ull, 129ull, 4095ull, 4096ull, 4097ull, 0xFFFFFFFFull})
        for (uint64_t wv : {1ull, 3ull, 4ull, 5ull, 1563ull, 1ull << 24}) {
            const bigsi::TallyPlan p = bigsi::plan_tally(n, wv);
            CHECK(p.word_groups * (bigsi::kBlock / 64) >= wv && (p.word_groups - 1) * (bigsi::kBlock / 64) < wv, "word groups of %llu words", (unsigned long long)wv);
            CHECK(p.tiles * p.tile >= n && (p.tiles - 1) * p.tile < n, "tiles of %llu queries", (unsigned long long)n);
            CHECK(p.grid == p.word_groups * p.tiles && (p.too_large != 0) == (p.grid > 0x7FFFFFFFull), "grid %llu", (unsigned long long)p.grid);
        }
    for (uint64_t n : {1ull, 4095ull, 4096ull, 4097ull, 9000ull})
        for (uint64_t wv_pad : {2ull, 1564ull, 8192ull, 1ull << 20})
            for (uint32_t cb : {0u, 2u, 4u}) {
                std::vector<uint64_t> len(n);
                for (auto &l : len) l = rnd() % 400;
                chunk_shape(len, 31, wv_pad, cb);
            }
    std::vector<uint64_t> len(600, 2000 + 30);      // 2000 positions each: 2^20 lies inside sequence 524
    chunk_shape(len, 31, 2, 4);
    len[3] = (1ull << 20) + 500;                    // one sequence beyond the position bound: a chunk of its own
    chunk_shape(len, 31, 2, 4);
    len.assign(5, 10);                              // nothing but sequences shorter than k
    chunk_shape(len, 31, 2, 0);
}

static void twin(uint64_t m, uint64_t n_cols, uint32_t h, uint32_t k, uint64_t n_seqs, double threshold)
{
    bigsi_cpu_index *ix = nullptr;
    CHECK(bigsi_cpu_open(m, n_cols, n_cols, h, 0, &ix) == 0, "%s", bigsi_cpu_last_error());
    bigsi_hip_info info;
    CHECK(bigsi_cpu_get_info(ix, &info) == 0, "%s", bigsi_cpu_last_error());
    const uint64_t stride = info.row_stride_bytes;
    std::vector<uint8_t> rows(m * stride);
    for (auto &b : rows) b = (uint8_t)(rnd() | rnd());          // dense rows, junk behind num_cols included: hits at every threshold
    std::vector<uint64_t> ids(m);
    for (uint64_t r = 0; r < m; r++) ids[r] = r;
    CHECK(bigsi_cpu_set_rows(ix, ids.data(), m, rows.data(), stride) == 0, "%s", bigsi_cpu_last_error());
    std::string blob;
    std::vector<uint64_t> off(n_seqs + 1, 0);
    for (uint64_t i = 0; i < n_seqs; i++) {
        const uint64_t len = i == 1 ? k - 1 : k + rnd() % 9;
        for (uint64_t j = 0; j < len; j++) blob.push_back("ACGT"[rnd() & 3]);
        off[i + 1] = blob.size();
    }
    std::vector<uint64_t> hit(n_cols + 1, 0xABABABABABABABABull), found(n_cols + 1, 0xABABABABABABABABull);
    uint64_t totals[4] = {9, 9, 9, 9};
    CHECK(bigsi_cpu_search_tally(ix, blob.data(), off.data(), n_seqs, k, threshold, hit.data(), found.data(), n_cols - 1, totals) == BIGSI_ERR_CAPACITY, "capacity");
    CHECK(hit[0] == 0xABABABABABABABABull && totals[0] == 9, "a refused call wrote its outputs");
    CHECK(bigsi_cpu_search_tally(ix, blob.data(), off.data(), n_seqs, k, 1.5, hit.data(), found.data(), n_cols, totals) == BIGSI_ERR_INVALID, "threshold 1.5");
    CHECK(bigsi_cpu_search_tally(ix, blob.data(), off.data(), n_seqs, k, threshold, nullptr, found.data(), n_cols, totals) == BIGSI_ERR_INVALID, "NULL");
    CHECK(bigsi_cpu_search_tally(ix, blob.data(), off.data(), n_seqs, k, threshold, hit.data(), found.data(), n_cols, totals) == 0, "%s", bigsi_cpu_last_error());
    CHECK(hit[n_cols] == 0xABABABABABABABABull && found[n_cols] == 0xABABABABABABABABull, "wrote behind num_cols");
    // against the twin's own search, sequence by sequence
    std::vector<uint64_t> want_hit(n_cols, 0), want_found(n_cols, 0);
    uint64_t want[4] = {0, 0, 0, 0};
    for (uint64_t i = 0; i < n_seqs; i++) {
        uint32_t nk, nu, mk;
        std::vector<uint64_t> hoff(2);
        std::vector<uint32_t> col(n_cols), cnt(n_cols);
        const uint64_t one[2] = {off[i], off[i + 1]};
        CHECK(bigsi_cpu_search_batch(ix, blob.data(), one, 1, k, threshold < 0 ? 0.0 : threshold, 0, &nk, &nu, &mk, hoff.data(), col.data(), cnt.data(), n_cols) == 0, "%s",
              bigsi_cpu_last_error());
        if (nu == 0) { want[2]++; continue; }
        want[0]++;
        want[1] += nu;
        if (hoff[1]) want[3]++;
        for (uint64_t j = 0; j < hoff[1]; j++) { want_hit[col[j]]++; want_found[col[j]] += cnt[j]; }
    }
    CHECK(memcmp(want, totals, sizeof want) == 0, "totals %llu %llu %llu %llu", (unsigned long long)totals[0], (unsigned long long)totals[1], (unsigned long long)totals[2], (unsigned long long)totals[3]);
    CHECK(memcmp(want_hit.data(), hit.data(), n_cols * 8) == 0 && memcmp(want_found.data(), found.data(), n_cols * 8) == 0, "the sums of %llu columns", (unsigned long long)n_cols);
    CHECK(n_seqs < 2 || totals[2] >= 1, "no sequence shorter than k");
    CHECK(bigsi_cpu_close(ix) == 0, "%s", bigsi_cpu_last_error());
}

int main()
{
    planners();
    for (uint64_t n_cols : {1ull, 63ull, 64ull, 65ull, 129ull, 200ull})
        for (double t : {1.0, 0.5, 0.0, -1.0})
            for (uint64_t n_seqs : {1ull, 2ull, 9ull}) twin(97, n_cols, 2, 5, n_seqs, t);
    printf("tally planners and twin: ok\n");
    return 0;
}
