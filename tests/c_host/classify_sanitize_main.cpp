// A stand-alone program (its own main) that drives the host planner of the read classification (plan_classify, classify_bad_column,
// bigsi_amd/csrc/bigsi_launch.hpp) and the CPU twin's bigsi_cpu_classify (bigsi_amd/cpu/bigsi_cpu.cpp) over odd shapes, checks the
// planner's invariants and the twin against the twin's own per-sequence search, and is meant to be built with
// -fsanitize=address,undefined and run on the CPU: tests/test_classify_host.py compiles it together with bigsi_cpu.cpp and runs it.
// Nothing sanitized is loaded into Python.
// Test infrastructure only: nothing in the product loads this file.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../bigsi_amd/csrc/bigsi_launch.hpp"
#include "bigsi_cpu_classify.h"

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
    for (uint64_t n : {0ull, 1ull, 4096ull, 0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFFull})
        for (uint64_t wv : {1ull, 13ull, 1563ull, 1ull << 26})
            for (uint64_t g : {0ull, 1ull, 2ull, 3ull, 100ull, 4095ull, 4096ull, 4097ull, 1ull << 40}) {
                const bigsi::ClassifyPlan p = bigsi::plan_classify(n, wv, g);
                CHECK(p.block == (uint32_t)bigsi::kBlock && p.grid == n, "one workgroup per query");
                CHECK((p.too_large != 0) == (n > 0x7FFFFFFFull), "grid of %llu", (unsigned long long)n);
                CHECK(p.bad_groups == (g == 0 || g > bigsi::kClassifyMaxGroups), "%llu groups", (unsigned long long)g);
                if (!p.bad_groups) {
                    CHECK(p.table_bytes >= g * 12 && p.table_bytes < g * 12 + 16 && p.table_bytes % 16 == 0, "table of %llu groups", (unsigned long long)g);
                    CHECK(p.lds_bytes == p.table_bytes + (bigsi::kBlock / 64) * 24 && p.lds_bytes <= 64 * 1024, "LDS of %llu groups", (unsigned long long)g);
                }
            }
    std::vector<uint32_t> g(130, 0);
    CHECK(bigsi::classify_bad_column(g.data(), g.size(), 1) == g.size(), "all zero");
    g[129] = 1;
    CHECK(bigsi::classify_bad_column(g.data(), g.size(), 1) == 129 && bigsi::classify_bad_column(g.data(), g.size(), 2) == g.size(), "the last column");
    g[129] = bigsi::kClassifyNoGroup;
    g[0] = 0xFFFFFFFEu;
    CHECK(bigsi::classify_bad_column(g.data(), g.size(), 4096) == 0 && bigsi::classify_bad_column(g.data(), 0, 1) == 0, "the first column; no columns");
}

static void twin(uint64_t m, uint64_t n_cols, uint32_t h, uint32_t k, uint64_t n_seqs, double threshold, uint32_t n_groups)
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
    std::vector<uint32_t> group_of(n_cols);
    for (uint64_t c = 0; c < n_cols; c++) group_of[c] = rnd() % 5 == 0 ? BIGSI_CLASSIFY_NONE : (uint32_t)(rnd() % n_groups);
    std::vector<bigsi_hip_classify_record> rec(n_seqs + 1);
    memset(rec.data(), 0xAB, rec.size() * sizeof rec[0]);
    const bigsi_hip_classify_record guard = rec[n_seqs];
    auto call = [&](double t, const uint32_t *g, uint64_t n_entries, uint32_t groups, bigsi_hip_classify_record *out) {
        return bigsi_cpu_classify(ix, blob.data(), off.data(), n_seqs, k, t, g, n_entries, groups, out);
    };
    CHECK(call(1.5, group_of.data(), n_cols, n_groups, rec.data()) == BIGSI_ERR_INVALID, "threshold 1.5");
    CHECK(call(threshold, nullptr, n_cols, n_groups, rec.data()) == BIGSI_ERR_INVALID && call(threshold, group_of.data(), n_cols, n_groups, nullptr) == BIGSI_ERR_INVALID, "NULL");
    CHECK(call(threshold, group_of.data(), n_cols + 1, n_groups, rec.data()) == BIGSI_ERR_INVALID, "n_entries");
    CHECK(call(threshold, group_of.data(), n_cols, 0, rec.data()) == BIGSI_ERR_INVALID && call(threshold, group_of.data(), n_cols, 4097, rec.data()) == BIGSI_ERR_INVALID, "n_groups");
    {
        std::vector<uint32_t> bad(group_of);
        bad[n_cols - 1] = n_groups;
        CHECK(call(threshold, bad.data(), n_cols, n_groups, rec.data()) == BIGSI_ERR_INVALID, "a group id of n_groups");
    }
    CHECK(memcmp(&rec[0], &guard, sizeof guard) == 0, "a refused call wrote its output");
    CHECK(call(threshold, group_of.data(), n_cols, n_groups, rec.data()) == 0, "%s", bigsi_cpu_last_error());
    CHECK(memcmp(&rec[n_seqs], &guard, sizeof guard) == 0, "wrote behind n_seqs");
    // against the twin's own search, sequence by sequence, every group weighed on its own
    bool some_hit = false;
    for (uint64_t i = 0; i < n_seqs; i++) {
        uint32_t nk, nu, mk;
        std::vector<uint64_t> hoff(2);
        std::vector<uint32_t> col(n_cols), cnt(n_cols);
        const uint64_t one[2] = {off[i], off[i + 1]};
        CHECK(bigsi_cpu_search_batch(ix, blob.data(), one, 1, k, threshold < 0 ? 0.0 : threshold, 0, &nk, &nu, &mk, hoff.data(), col.data(), cnt.data(), n_cols) == 0, "%s",
              bigsi_cpu_last_error());
        const bigsi_hip_classify_record &r = rec[i];
        if (nu == 0) {
            CHECK(r.num_unique == 0 && r.min_kmers == 0 && r.groups_hit == 0 && r.samples_hit == 0 && r.best_group == BIGSI_CLASSIFY_NONE && r.best_found == 0 &&
                      r.best_colour == BIGSI_CLASSIFY_NONE && r.best_samples_hit == 0 && r.second_group == BIGSI_CLASSIFY_NONE && r.second_colour == BIGSI_CLASSIFY_NONE,
                  "the record of a sequence without k-mers");
            continue;
        }
        CHECK(r.num_unique == nu && r.min_kmers == mk, "num_unique / min_kmers of sequence %llu", (unsigned long long)i);
        uint32_t groups = 0, samples = 0;
        struct Place { uint32_t g, found, colour, n; };
        std::vector<Place> hit;
        for (uint32_t g = 0; g < n_groups; g++) {
            Place p{g, 0, BIGSI_CLASSIFY_NONE, 0};
            for (uint64_t j = 0; j < hoff[1]; j++)
                if (group_of[col[j]] == g) {
                    if (p.n == 0 || cnt[j] > p.found) { p.found = cnt[j]; p.colour = col[j]; }
                    p.n++;
                }
            if (p.n) { groups++; samples += p.n; hit.push_back(p); }
        }
        Place want[2] = {{BIGSI_CLASSIFY_NONE, 0, BIGSI_CLASSIFY_NONE, 0}, {BIGSI_CLASSIFY_NONE, 0, BIGSI_CLASSIFY_NONE, 0}};
        for (int place = 0; place < 2; place++) {
            int best = -1;
            for (size_t x = 0; x < hit.size(); x++)
                if (hit[x].g != want[0].g && (best < 0 || hit[x].found > hit[(size_t)best].found)) best = (int)x;      // (ascending ids: the first maximum is the lowest id)
            if (best >= 0) want[place] = hit[(size_t)best];
        }
        CHECK(r.groups_hit == groups && r.samples_hit == samples, "groups_hit / samples_hit of sequence %llu", (unsigned long long)i);
        CHECK(r.best_group == want[0].g && r.best_found == want[0].found && r.best_colour == want[0].colour && r.best_samples_hit == want[0].n, "the best group of sequence %llu",
              (unsigned long long)i);
        CHECK(r.second_group == want[1].g && r.second_found == want[1].found && r.second_colour == want[1].colour && r.second_samples_hit == want[1].n,
              "the second group of sequence %llu", (unsigned long long)i);
        some_hit = some_hit || groups > 0;
    }
    CHECK(threshold > 0.0 || some_hit || n_cols < 8, "at threshold 0 every grouped column is a hit, yet no sequence hit any group");
    CHECK(bigsi_cpu_close(ix) == 0, "%s", bigsi_cpu_last_error());
}

int main()
{
    planner();
    for (uint64_t n_cols : {1ull, 63ull, 64ull, 65ull, 129ull, 200ull})
        for (double t : {1.0, 0.5, 0.0, -1.0})
            for (uint64_t n_seqs : {1ull, 2ull, 9ull})
                for (uint32_t n_groups : {1u, 7u, 4096u}) twin(97, n_cols, 2, 5, n_seqs, t, n_groups);
    printf("classify planner and twin: ok\n");
    return 0;
}
