// A stand-alone program (its own main) that drives the host half of the band sweep (bigsi_amd/csrc/bigsi_launch.hpp): the window
// bounds (band_window), the search a wavefront makes for its part of a bucket-sorted row list (band_lower_bound) and the planner
// (plan_band_sweep).  It replays a band's windows over seeded lists the way the kernel does -- search, take the sub-range, move on --
// and checks that every list entry is visited exactly once, whatever the number of windows.  Meant to be built with
// -fsanitize=address,undefined and run on the CPU: tests/test_band_plan_host.py compiles and runs it.  Nothing sanitized is loaded
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

// a list as the sorts leave it: ascending in (id >> shift), shuffled inside a bucket, duplicates allowed
static std::vector<uint64_t> bucket_sorted(uint64_t m, uint64_t n, uint32_t shift)
{
    std::vector<uint64_t> r(n);
    for (auto &x : r) x = rnd() % m;
    std::sort(r.begin(), r.end());
    for (size_t a = 0; a < r.size();) {
        size_t b = a;
        while (b < r.size() && (r[b] >> shift) == (r[a] >> shift)) b++;
        for (size_t i = b - 1; i > a; i--) std::swap(r[i], r[a + rnd() % (i - a + 1)]);
        a = b;
    }
    return r;
}

static void sweep(uint64_t m, uint64_t n, uint32_t W, uint64_t buckets)
{
    const uint32_t shift = bigsi::sort_shift(m, buckets);
    CHECK(((m - 1) >> shift) < buckets && (shift == 0 || ((m - 1) >> (shift - 1)) >= buckets), "shift %u for %llu rows", shift, (unsigned long long)m);
    const std::vector<uint64_t> r = bucket_sorted(m, n, shift);
    uint64_t next_row = 0, next_item = 0;
    for (uint32_t w = 0; w < W; w++) {
        const bigsi::BandWindow x = bigsi::band_window(m, w, W, shift);
        CHECK(x.lo == next_row && x.lo <= x.hi && x.hi <= m, "window %u of %u over %llu rows", w, W, (unsigned long long)m);
        CHECK(x.lo == m || x.lo % (1ull << shift) == 0, "window %u starts inside a bucket", w);
        next_row = x.hi;
        const uint64_t a = bigsi::band_lower_bound(r.data(), r.size(), x.lo);
        const uint64_t b = a + bigsi::band_lower_bound(r.data() + a, r.size() - a, x.hi);
        CHECK(a == next_item && b <= r.size(), "window %u takes [%llu, %llu) after %llu", w, (unsigned long long)a, (unsigned long long)b, (unsigned long long)next_item);
        for (uint64_t i = a; i < b; i++) CHECK(r[i] >= x.lo && r[i] < x.hi, "item %llu outside window %u", (unsigned long long)i, w);
        next_item = b;
    }
    CHECK(next_row == m && next_item == r.size(), "the windows end at row %llu, item %llu", (unsigned long long)next_row, (unsigned long long)next_item);
}

static void planner(uint32_t n_seqs, uint64_t wv, uint64_t max_pos, uint32_t h, uint64_t m, bool forced, uint32_t fw, uint32_t fs)
{
    const bigsi::BandSweepPlan p = bigsi::plan_band_sweep(bigsi::RowAndInput{n_seqs, wv, max_pos, h, true, false, false, false}, m, forced, fw, fs);
    if (!p.taken) {
        CHECK(p.n_launches == 0, "launches of a plan not taken");
        return;
    }
    const uint64_t segs = (wv + 127) / 128;
    std::vector<uint32_t> next_window(segs + 2, 0);
    for (uint32_t i = 0; i < p.n_launches; i++) {
        const bigsi::BandLaunch l = p.launch(i);
        const bool tail = p.merge_tail && l.seg0 + 2 == segs;
        CHECK(l.nseg == (tail ? 2 : p.segs_per_launch) && l.seg0 % p.segs_per_launch == 0 && l.seg0 < segs && l.window < p.windows, "launch %u", i);
        CHECK(l.grid * 4 >= (uint64_t)n_seqs * l.nseg && l.grid <= 0x7FFFFFFFull, "grid of launch %u", i);
        for (uint32_t s = l.seg0; s < l.seg0 + l.nseg; s++) CHECK(next_window[s]++ == l.window, "segment %u meets window %u out of order", s, l.window);
    }
    for (uint64_t s = 0; s < segs; s++) CHECK(next_window[s] == p.windows, "segment %llu saw %u windows", (unsigned long long)s, next_window[s]);
}

int main()
{
    for (uint64_t m : {1ull, 2ull, 7ull, 1009ull, 8192ull, 8193ull, 100003ull, 10000000ull})
        for (uint64_t n : {0ull, 1ull, 2ull, 300ull, 3880ull})
            for (uint32_t W : {1u, 2u, 3u, 16u, 64u, 2000u})
                for (uint64_t buckets : {2ull, 512ull, 8192ull}) sweep(m, n, W, buckets);
    sweep(1009, 300, 65536, 8192);
    for (uint32_t n_seqs : {1u, 7u, 301u, 4096u, 4097u, 8192u, 8193u})
        for (uint64_t wv : {1ull, 128ull, 129ull, 130ull, 1563ull})
            for (uint32_t fw : {0u, 1u, 3u, 2000u})
                for (uint32_t fs : {0u, 1u, 2u}) {
                    planner(n_seqs, wv, 970, 4, 10000000, false, fw, fs);
                    planner(n_seqs, wv, 70, 3, 1009, true, fw, fs);
                }
    printf("band windows, search and planner: ok\n");
    return 0;
}
