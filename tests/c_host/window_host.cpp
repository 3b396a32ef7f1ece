// CPU pin of plan_window_search (bigsi_amd/csrc/bigsi_launch.hpp): the launch shape of the windowed search's sweep -- segment length,
// plane bucket, grid, the per-segment maxima's size, the refusals -- compiled here as plain host C++.
// tests/test_window_host.py loads it and checks the cover of the window starts, the buckets and the sizes.
// Test infrastructure only: nothing in the product loads this file.
#include "../../bigsi_amd/csrc/bigsi_launch.hpp"

extern "C" {

// out[]: max_we, planes, seg_starts, tiles, n_segs, waves, grid, wvp, partial_bytes, steps_per_iter, grid_too_large, partial_too_large,
//        kWindowWaves, kWindowPartialBytes, kWindowMax
// segs (when non-null): up to seg_capacity entries of {q, a, b, we}; seg_off (when non-null): n_seqs + 1 entries
void window_host_plan(const uint32_t *n, uint32_t n_seqs, uint32_t window, uint64_t wv, uint32_t h, uint64_t forced_starts, uint64_t partial_cap,
                      uint64_t *out, uint32_t *segs, uint64_t seg_capacity, uint64_t *seg_off)
{
    const bigsi::WindowPlan p = bigsi::plan_window_search(n, n_seqs, window, wv, h, forced_starts, partial_cap);
    const uint64_t v[15] = {p.max_we, p.planes, p.seg_starts, p.tiles, p.n_segs, p.waves, p.grid, p.wvp, p.partial_bytes, p.steps_per_iter,
                            p.grid_too_large, p.partial_too_large, bigsi::kWindowWaves, bigsi::kWindowPartialBytes, bigsi::kWindowMax};
    for (int i = 0; i < 15; i++) out[i] = v[i];
    if (segs)
        for (uint64_t i = 0; i < p.segs.size() && i < seg_capacity; i++) {
            segs[4 * i] = p.segs[i].q;
            segs[4 * i + 1] = p.segs[i].a;
            segs[4 * i + 2] = p.segs[i].b;
            segs[4 * i + 3] = p.segs[i].we;
        }
    if (seg_off)
        for (uint32_t q = 0; q <= n_seqs; q++) seg_off[q] = p.seg_off[q];
}

uint32_t window_host_bucket(uint32_t we) { return bigsi::window_plane_bucket(we); }
uint32_t window_host_bit_width(uint32_t x) { return bigsi::window_bit_width(x); }

}
