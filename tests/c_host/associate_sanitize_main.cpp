// A stand-alone program (its own main) that drives the host planner of the group association (plan_associate, and the group_of
// validation it shares with the classification, classify_bad_column; bigsi_amd/csrc/bigsi_launch.hpp) and the CPU twin's
// bigsi_cpu_associate (bigsi_amd/cpu/bigsi_cpu.cpp) over odd shapes at the width edges, checks the planner's invariants and the twin
// against the twin's own per-sequence search, and is meant to be built with -fsanitize=address,undefined and run on the CPU:
// tests/test_associate_host.py compiles it together with bigsi_cpu.cpp and runs it.  Nothing sanitized is loaded into Python.
// Test infrastructure only: nothing in the product loads this file.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../bigsi_amd/csrc/bigsi_launch.hpp"
#include "bigsi_cpu_associate.h"

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

static void planner()
{
    const uint64_t Q = bigsi::kAssociateQueries, GB = bigsi::kAssociateGroupBlock;
    for (uint64_t n : {0ull, 1ull, 3ull, 4ull, 5ull, 4096ull, 4ull * 0x7FFFFFFFull, 4ull * 0x7FFFFFFFull + 1, 0xFFFFFFFFFFull})
        for (uint64_t wv : {1ull, 3ull, 4ull, 5ull, 13ull, 1563ull, 1ull << 26, 1ull << 34})
            for (uint64_t g : {0ull, 1ull, 2ull, 7ull, 8ull, 9ull, 63ull, 64ull, 65ull, 1ull << 40}) {
                const bigsi::AssociatePlan p = bigsi::plan_associate(n, wv, g);
                CHECK(p.block == (uint32_t)bigsi::kBlock && p.grid * Q >= n && (p.grid == 0 || (p.grid - 1) * Q < n), "%llu queries", (unsigned long long)n);
                CHECK(p.mask_grid * 4 >= wv && (p.mask_grid - 1) * 4 < wv, "%llu words", (unsigned long long)wv);
                CHECK((p.too_large != 0) == (p.grid > 0x7FFFFFFFull || p.mask_grid > 0x7FFFFFFFull), "too_large");
                CHECK(p.bad_groups == (g == 0 || g > bigsi::kAssociateMaxGroups), "%llu groups", (unsigned long long)g);
                CHECK(p.lds_bytes == 4 * Q * (GB + 1) * 4 && p.lds_bytes <= 64 * 1024, "LDS");
                if (!p.bad_groups) CHECK(p.passes * GB >= g && (p.passes - 1) * GB < g && p.mask_bytes == g * wv * 8, "passes / masks of %llu groups", (unsigned long long)g);
            }
    std::vector<uint32_t> g(130, 0);
    CHECK(bigsi::classify_bad_column(g.data(), g.size(), 1) == g.size(), "all zero");
    g[129] = 64;
    CHECK(bigsi::classify_bad_column(g.data(), g.size(), 64) == 129 && bigsi::classify_bad_column(g.data(), g.size(), 65) == g.size(), "the last column");
    g[129] = BIGSI_ASSOCIATE_NONE;
    CHECK(bigsi::classify_bad_column(g.data(), g.size(), 1) == g.size(), "BIGSI_ASSOCIATE_NONE is no group");
    CHECK(BIGSI_ASSOCIATE_NONE == bigsi::kAssociateNoGroup && BIGSI_ASSOCIATE_NONE == bigsi::kClassifyNoGroup && BIGSI_ASSOCIATE_MAX_GROUPS == bigsi::kAssociateMaxGroups, "constants");
}

static void twin(uint64_t m, uint64_t n_cols, uint32_t h, uint32_t k, uint64_t n_seqs, double threshold, uint32_t n_groups)
{
    bigsi_cpu_index *ix = nullptr;
    CHECK(bigsi_cpu_open(m, n_cols, n_cols, h, 0, &ix) == 0, "%s", bigsi_cpu_last_error());
    bigsi_hip_info inf;
    CHECK(bigsi_cpu_get_info(ix, &inf) == 0, "%s", bigsi_cpu_last_error());
    const uint64_t stride = inf.row_stride_bytes;
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
    std::vector<uint32_t> group_of(n_cols);
    for (uint64_t c = 0; c < n_cols; c++) group_of[c] = rnd() % 5 == 0 ? BIGSI_ASSOCIATE_NONE : (uint32_t)(rnd() % n_groups);
    std::vector<uint32_t> counts((n_seqs + 1) * n_groups);
    std::vector<bigsi_hip_associate_info> info(n_seqs + 1);
    memset(counts.data(), 0xAB, counts.size() * 4);
    memset(info.data(), 0xAB, info.size() * sizeof info[0]);
    const bigsi_hip_associate_info guard = info[n_seqs];
    auto call = [&](double t, const uint32_t *g, uint64_t n_entries, uint32_t groups, uint32_t *c, bigsi_hip_associate_info *o) {
        return bigsi_cpu_associate(ix, blob.data(), off.data(), n_seqs, k, t, g, n_entries, groups, c, o);
    };
    CHECK(call(1.5, group_of.data(), n_cols, n_groups, counts.data(), info.data()) == BIGSI_ERR_INVALID, "threshold 1.5");
    CHECK(call(threshold, nullptr, n_cols, n_groups, counts.data(), info.data()) == BIGSI_ERR_INVALID, "NULL group_of");
    CHECK(call(threshold, group_of.data(), n_cols, n_groups, nullptr, info.data()) == BIGSI_ERR_INVALID, "NULL counts");
    CHECK(call(threshold, group_of.data(), n_cols, n_groups, counts.data(), nullptr) == BIGSI_ERR_INVALID, "NULL info");
    CHECK(call(threshold, group_of.data(), n_cols + 1, n_groups, counts.data(), info.data()) == BIGSI_ERR_INVALID, "n_entries");
    CHECK(call(threshold, group_of.data(), n_cols, 0, counts.data(), info.data()) == BIGSI_ERR_INVALID, "no groups");
    CHECK(call(threshold, group_of.data(), n_cols, 65, counts.data(), info.data()) == BIGSI_ERR_INVALID && strstr(bigsi_cpu_last_error(), "BIGSI_ASSOCIATE_MAX_GROUPS"), "65 groups");
    {
        std::vector<uint32_t> bad(group_of);
        bad[n_cols - 1] = n_groups;
        CHECK(call(threshold, bad.data(), n_cols, n_groups, counts.data(), info.data()) == BIGSI_ERR_INVALID, "a group id of n_groups");
    }
    CHECK(memcmp(&info[0], &guard, sizeof guard) == 0 && counts[0] == 0xABABABABu, "a refused call wrote its output");
    CHECK(call(threshold, group_of.data(), n_cols, n_groups, counts.data(), info.data()) == 0, "%s", bigsi_cpu_last_error());
    CHECK(memcmp(&info[n_seqs], &guard, sizeof guard) == 0, "wrote behind n_seqs");
    for (uint32_t g = 0; g < n_groups; g++) CHECK(counts[n_seqs * n_groups + g] == 0xABABABABu, "wrote behind the counts");
    // against the twin's own search, sequence by sequence, every group counted on its own
    std::vector<uint64_t> sizes(n_groups, 0);
    for (uint64_t c = 0; c < n_cols; c++)
        if (group_of[c] != BIGSI_ASSOCIATE_NONE) sizes[group_of[c]]++;
    for (uint64_t i = 0; i < n_seqs; i++) {
        uint32_t nk, nu, mk;
        std::vector<uint64_t> hoff(2);
        std::vector<uint32_t> col(n_cols), cnt(n_cols);
        const uint64_t one[2] = {off[i], off[i + 1]};
        CHECK(bigsi_cpu_search_batch(ix, blob.data(), one, 1, k, threshold < 0 ? 0.0 : threshold, 0, &nk, &nu, &mk, hoff.data(), col.data(), cnt.data(), n_cols) == 0, "%s",
              bigsi_cpu_last_error());
        const bigsi_hip_associate_info &r = info[i];
        if (nu == 0) {
            CHECK(r.num_unique == 0 && r.min_kmers == 0 && r.samples_hit == 0 && r.grouped_hit == 0, "the info of a sequence without k-mers");
            for (uint32_t g = 0; g < n_groups; g++) CHECK(counts[i * n_groups + g] == 0, "the counts of a sequence without k-mers");
            continue;
        }
        CHECK(r.num_unique == nu && r.min_kmers == mk && r.samples_hit == hoff[1], "num_unique / min_kmers / samples_hit of sequence %llu", (unsigned long long)i);
        uint64_t grouped = 0;
        for (uint32_t g = 0; g < n_groups; g++) {
            uint32_t n = 0;
            for (uint64_t j = 0; j < hoff[1]; j++) n += group_of[col[j]] == g;
            CHECK(counts[i * n_groups + g] == n, "group %u of sequence %llu", g, (unsigned long long)i);
            if (threshold <= 0.0) CHECK(n == sizes[g], "at threshold 0 a group's count is its size (group %u)", g);
            grouped += n;
        }
        CHECK(r.grouped_hit == grouped, "grouped_hit of sequence %llu", (unsigned long long)i);
    }
    CHECK(bigsi_cpu_close(ix) == 0, "%s", bigsi_cpu_last_error());
}

int main()
{
    planner();
    for (uint64_t n_cols : {1ull, 63ull, 64ull, 65ull, 127ull, 129ull, 200ull})
        for (double t : {1.0, 0.5, 0.0, -1.0})
            for (uint64_t n_seqs : {1ull, 2ull, 9ull})
                for (uint32_t n_groups : {1u, 7u, 64u}) twin(97, n_cols, 2, 5, n_seqs, t, n_groups);
    printf("associate planner and twin: ok\n");
    return 0;
}
