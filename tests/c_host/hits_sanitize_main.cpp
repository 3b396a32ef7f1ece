// A stand-alone program (its own main) that drives the launch rule of the hit-list compaction and the size of the pinned export
// (bigsi_amd/csrc/bigsi_launch.hpp: plan_hits, export_spec) over a seeded sweep the way k_hits_totals / k_hits_write walk a plan:
// workgroup g marks its items [g ipb, min((g + 1) ipb, n)) in an array of exactly n entries on the heap -- every item must be owned
// once, no workgroup may be empty, exactly one workgroup may end at n (the one that writes the grand total) -- and the threads of the
// single-workgroup body mark their words chunks t .. chunks t + chunks - 1 of a vector of exactly wv words.  Meant to be built with
// -fsanitize=address,undefined and run on the CPU: tests/test_hits_plan_host.py compiles and runs it.  Nothing sanitized is loaded
// into Python.
// Test infrastructure only: nothing in the product loads this file.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../bigsi_amd/csrc/bigsi_launch.hpp"

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

// the plan's arithmetic alone (any n up to the host's bound of 2^31 - 1 items)
static void check_plan(uint64_t n, uint32_t n_shards)
{
    const bigsi::HitsPlan p = bigsi::plan_hits(n, n_shards);
    const unsigned long long nn = n;
    CHECK(p.ipb >= 1 && p.groups >= 1 && p.groups <= bigsi::kHitsMaxGroups, "%llu items: ipb %u, groups %llu", nn, p.ipb, (unsigned long long)p.groups);
    if (n) CHECK(p.groups * p.ipb >= n && n > (p.groups - 1) * p.ipb, "%llu items: ipb %u, groups %llu", nn, p.ipb, (unsigned long long)p.groups);
    CHECK((p.groups == 1) == (n <= bigsi::kHitsOneGroupItems), "%llu items: groups %llu", nn, (unsigned long long)p.groups);
    CHECK(p.single == (p.groups == 1 && n_shards == 1), "%llu items on %u shards: single %d", nn, n_shards, (int)p.single);
    if (n > bigsi::kHitsOneGroupItems) CHECK(p.ipb == ceil_div(n, bigsi::kHitsMaxGroups), "%llu items: ipb %u", nn, p.ipb);
}

// the walk of the general body over an array of exactly n items
static void walk_groups(uint64_t n)
{
    const bigsi::HitsPlan p = bigsi::plan_hits(n);
    std::vector<uint8_t> owned(n, 0);
    uint64_t ends_at_n = 0;
    for (uint64_t g = 0; g < p.groups; g++) {
        const uint64_t i0 = g * p.ipb, i1 = i0 + p.ipb < n ? i0 + p.ipb : n;
        CHECK(n == 0 || i0 < i1, "%llu items: workgroup %llu is empty", (unsigned long long)n, (unsigned long long)g);
        for (uint64_t i = i0; i < i1; i++) owned[i]++;
        ends_at_n += i1 == n;
    }
    for (uint64_t i = 0; i < n; i++) CHECK(owned[i] == 1, "%llu items: item %llu owned %d times", (unsigned long long)n, (unsigned long long)i, (int)owned[i]);
    CHECK(ends_at_n == 1, "%llu items: %llu workgroups write the grand total", (unsigned long long)n, (unsigned long long)ends_at_n);
}

// the walk of the single-workgroup body over one vector of exactly wv words
static void walk_threads(uint64_t wv)
{
    const uint32_t chunks = (uint32_t)ceil_div(wv, bigsi::kBlock);
    CHECK(bigsi::plan_hits(chunks).single == (chunks <= bigsi::kHitsOneGroupItems), "%llu words", (unsigned long long)wv);
    if (chunks > bigsi::kHitsOneGroupItems) return;
    std::vector<uint8_t> owned(wv, 0);
    for (uint32_t t = 0; t < (uint32_t)bigsi::kBlock; t++)
        for (uint32_t j = 0; j < bigsi::kHitsOneGroupItems; j++) {
            const uint64_t w = (uint64_t)t * chunks + j;
            if (j < chunks && w < wv) owned[w]++;
        }
    for (uint64_t w = 0; w < wv; w++) CHECK(owned[w] == 1, "%llu words: word %llu owned %d times", (unsigned long long)wv, (unsigned long long)w, (int)owned[w]);
}

int main()
{
    uint64_t plans = 0;
    for (uint64_t n = 0; n <= 5000; n++, plans++) { check_plan(n, 1); check_plan(n, 3); walk_groups(n); }
    for (uint64_t n : {65535ull, 65536ull, 65537ull, 1048575ull, 1048576ull, 1048577ull, 0x7FFFFFFEull, 0x7FFFFFFFull}) { check_plan(n, 1); plans++; }
    for (int i = 0; i < 20000; i++, plans++) {
        const uint64_t n = rnd() % 0x80000000ull >> (rnd() % 31);
        check_plan(n, 1 + (uint32_t)(rnd() % 8));
        if (n <= 3000000) walk_groups(n);
    }
    for (uint64_t wv = 1; wv <= 4400; wv++) walk_threads(wv);
    // the export: never more than the lists hold nor than the ceiling, the floor when the lists hold it, 16 per sequence in between
    for (int i = 0; i < 20000; i++) {
        const uint64_t n = i < 100 ? (uint64_t)i : (rnd() & 0xFFFFFFFFull) >> (rnd() % 32), cap = i % 7 == 0 ? bigsi::kHitsInitialCapacity : rnd() >> (rnd() % 64);
        const uint64_t s = bigsi::export_spec(n, cap);
        CHECK(s <= cap && s <= bigsi::kExportSpecMax, "spec(%llu, %llu) = %llu", (unsigned long long)n, (unsigned long long)cap, (unsigned long long)s);
        CHECK(s == cap || s == bigsi::kExportSpecMax || s == bigsi::kExportSpecMin || s == bigsi::kExportSpecPerSeq * n, "spec(%llu, %llu) = %llu",
              (unsigned long long)n, (unsigned long long)cap, (unsigned long long)s);
        if (cap >= bigsi::kExportSpecMin) CHECK(s >= bigsi::kExportSpecMin, "spec(%llu, %llu) = %llu", (unsigned long long)n, (unsigned long long)cap, (unsigned long long)s);
    }
    CHECK(plans > 25000, "only %llu plans", (unsigned long long)plans);
    printf("hit-list plan, its walks and the export's size: ok\n");
    return 0;
}
