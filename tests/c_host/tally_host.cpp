// CPU pin of plan_tally and plan_tally_chunks (bigsi_amd/csrc/bigsi_launch.hpp): the launch shape of the query-set tally's kernels and
// the cuts of bigsi_hip_tally_add_stream's device batches, compiled here as plain host C++.  tests/test_tally_host.py loads it and
// checks both against a plain Python restatement (tests/tally_ref.py).
// Test infrastructure only: nothing in the product loads this file.
#include "../../bigsi_amd/csrc/bigsi_launch.hpp"

extern "C" {

// out[]: kBlock, kTallyTile, kTallyLoads, kTallyTotalsTile, kTallyChunkSeqs, kTallyChunkPositions, kTallyCounterBytes
void tally_host_constants(uint64_t *out)
{
    const uint64_t v[7] = {(uint64_t)bigsi::kBlock, bigsi::kTallyTile, bigsi::kTallyLoads, bigsi::kTallyTotalsTile, bigsi::kTallyChunkSeqs,
                           bigsi::kTallyChunkPositions, bigsi::kTallyCounterBytes};
    for (int i = 0; i < 7; i++) out[i] = v[i];
}

// out[]: block, tile, word_groups, tiles, grid, totals_grid, too_large
void tally_host_plan(uint64_t n_seqs, uint64_t wv, uint64_t *out)
{
    const bigsi::TallyPlan p = bigsi::plan_tally(n_seqs, wv);
    const uint64_t v[7] = {p.block, p.tile, p.word_groups, p.tiles, p.grid, p.totals_grid, p.too_large};
    for (int i = 0; i < 7; i++) out[i] = v[i];
}

// the cuts (at most `capacity` of them are written); returns their number
uint64_t tally_host_chunks(const uint64_t *offsets, uint64_t n_seqs, uint32_t k, uint64_t wv_pad, uint32_t count_bytes, uint64_t *cuts, uint64_t capacity)
{
    const std::vector<uint64_t> c = bigsi::plan_tally_chunks(offsets, n_seqs, k, wv_pad, count_bytes);
    for (size_t i = 0; i < c.size() && i < capacity; i++) cuts[i] = c[i];
    return c.size();
}

}
