// CPU pin of bigsi_amd/csrc/bigsi_launch.hpp: the launch rule of a batch run (how the row-AND kernels are launched for a batch of
// queries), compiled here as plain host C++.  tests/test_abi_and_host.py loads it, pins the shapes DESIGN.md states and checks the
// rule's invariants over a seeded sweep of geometries.
// Test infrastructure only: nothing in the product loads this file.
#include "../../bigsi_amd/csrc/bigsi_launch.hpp"

extern "C" {

// head[]: too_large, slices, want_sorted, preset, P, count_bytes, planes_out, combine, deep, early, n_launches
// launches[]: up to `capacity` records of q0, q1, grid, block, tiles, slices, unroll, needs_preset
// Returns the number of launches of the plan.
uint64_t launch_host_plan(uint32_t n_seqs, uint64_t wv, uint64_t max_pos, uint32_t h, int exact, int no_sort, int early_exit,
                          int sparse_counts, uint64_t *head, uint64_t *launches, uint64_t capacity)
{
    const bigsi::RowAndPlan p = bigsi::plan_row_and(
        bigsi::RowAndInput{n_seqs, wv, max_pos, h, exact != 0, no_sort != 0, early_exit != 0, sparse_counts != 0});
    const uint64_t hd[11] = {p.too_large, p.slices, p.want_sorted, p.preset, (uint64_t)p.P, p.count_bytes, p.planes_out, p.combine,
                             p.deep, p.early, p.n_launches};
    for (int i = 0; i < 11; i++) head[i] = hd[i];
    for (uint32_t i = 0; i < p.n_launches && i < capacity; i++) {
        const bigsi::RowAndLaunch l = p.launch(i);
        const uint64_t rec[8] = {l.q0, l.q1, l.grid, l.block, l.tiles, l.slices, l.unroll, l.needs_preset};
        for (int j = 0; j < 8; j++) launches[8 * i + j] = rec[j];
    }
    return p.n_launches;
}

// k1_plan: out[] = route, hs_cap, sq_bytes, tab_mult, tab_cap, lds
void launch_host_k1_plan(uint32_t n_seqs, uint64_t max_pos, uint64_t max_len, int elements, int force_global, uint64_t *out)
{
    const bigsi::K1Plan p = bigsi::k1_plan(n_seqs, max_pos, max_len, elements != 0, force_global != 0);
    const uint64_t rec[6] = {(uint64_t)p.route, p.hs_cap, p.sq_bytes, p.tab_mult, p.tab_cap, p.lds};
    for (int i = 0; i < 6; i++) out[i] = rec[i];
}

// threads of k_sort_rows' workgroup: 256 or 1024
uint32_t launch_host_sort_rows_block(uint64_t max_pos, uint32_t h) { return bigsi::sort_rows_block(max_pos, h); }

// the one grid formula
uint64_t launch_host_grid(uint64_t n, uint64_t tiles, uint64_t slices) { return bigsi::row_and_grid(n, tiles, slices); }

// bigsi_exact_launch_queries of an index whose result vectors have `wv` words
uint32_t launch_host_exact_launch_queries(uint64_t wv) { return bigsi::exact_launch_queries(wv); }

}
