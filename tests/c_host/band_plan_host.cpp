// CPU pin of the band sweep's planner in bigsi_amd/csrc/bigsi_launch.hpp (plan_band_sweep, band_window, band_lower_bound, sort_shift),
// compiled here as plain host C++.  tests/test_band_plan_host.py loads it, pins the shapes the header states and checks the
// invariants over a seeded sweep of geometries.
// Test infrastructure only: nothing in the product loads this file.
#include "../../bigsi_amd/csrc/bigsi_launch.hpp"

extern "C" {

// head[]: taken, windows, segs_per_launch, seg_groups, unroll, grid, in_flight, n_launches, merge_tail
// launches[]: up to `capacity` records of seg0, nseg, window, grid, unroll
// Returns the number of launches of the plan.
uint64_t band_host_plan(uint32_t n_seqs, uint64_t wv, uint64_t max_pos, uint32_t h, int exact, int no_sort, int early_exit, uint64_t m,
                        int forced, uint32_t forced_windows, uint32_t forced_segs, uint64_t *head, uint64_t *launches, uint64_t capacity)
{
    const bigsi::BandSweepPlan p = bigsi::plan_band_sweep(
        bigsi::RowAndInput{n_seqs, wv, max_pos, h, exact != 0, no_sort != 0, early_exit != 0, false}, m, forced != 0, forced_windows, forced_segs);
    const uint64_t hd[9] = {p.taken, p.windows, p.segs_per_launch, p.seg_groups, p.unroll, p.grid, p.in_flight, p.n_launches, p.merge_tail};
    for (int i = 0; i < 9; i++) head[i] = hd[i];
    for (uint32_t i = 0; i < p.n_launches && i < capacity; i++) {
        const bigsi::BandLaunch l = p.launch(i);
        const uint64_t rec[5] = {l.seg0, l.nseg, l.window, l.grid, l.unroll};
        for (int j = 0; j < 5; j++) launches[5 * i + j] = rec[j];
    }
    return p.n_launches;
}

// the shipped constants: unroll, segments per launch, windows of a large batch, queries up to which a band is one window,
// break-even rho x 1000, in-flight cap in bytes, most windows, words of a last segment that rides with its neighbour,
// fewest queries
void band_host_constants(uint64_t *out)
{
    out[0] = bigsi::kBandUnroll;
    out[1] = bigsi::kBandSegs;
    out[2] = bigsi::kBandWindowsLarge;
    out[3] = bigsi::kBandOneWindowQueries;
    out[4] = (uint64_t)(bigsi::kBandMinRho * 1000.0 + 0.5);
    out[5] = bigsi::kBandInFlightCap;
    out[6] = bigsi::kBandMaxWindows;
    out[7] = bigsi::kBandTailWords;
    out[8] = bigsi::kBandMinQueries;
}

void band_host_window(uint64_t m, uint32_t w, uint32_t W, uint32_t shift, uint64_t *lo, uint64_t *hi)
{
    const bigsi::BandWindow x = bigsi::band_window(m, w, W, shift);
    *lo = x.lo;
    *hi = x.hi;
}

uint32_t band_host_sort_shift(uint64_t m, uint64_t buckets) { return bigsi::sort_shift(m, buckets); }

uint64_t band_host_lower_bound(const uint64_t *r, uint64_t n, uint64_t key) { return bigsi::band_lower_bound(r, n, key); }

}
