// CPU pin of plan_consensus_columns (bigsi_amd/csrc/bigsi_launch.hpp): the per-call tables of the consensus collapse -- dst_col, the
// destination column of every source bit as it lies in memory, live, the bits of every source word that count, the group sizes, the
// field width they ask for and need, the thresholds in the order the read-out holds a word's bits --, the launch shape and the
// destination window, compiled here as plain host C++.  tests/test_consensus_columns_host.py loads it and checks the tables against
// a bit-by-bit restatement of the row format and the window / LDS invariants over seeded shapes.
// Test infrastructure only: nothing in the product loads this file.
#include "../../bigsi_amd/csrc/bigsi_launch.hpp"

extern "C" {

// consts[]: kCollapseDropped, kCollapseWaves, kCollapseWindowWords, kCollapseLdsBytes, kCollapseLoads, kCollapseGathers, kBlock,
// kConsensusNever
void consensus_host_constants(uint64_t *consts)
{
    const uint64_t c[8] = {bigsi::kCollapseDropped,         bigsi::kCollapseWaves,           bigsi::kCollapseWindowWords, bigsi::kCollapseLdsBytes,
                           (uint64_t)bigsi::kCollapseLoads, (uint64_t)bigsi::kCollapseGathers, (uint64_t)bigsi::kBlock,   bigsi::kConsensusNever};
    for (int i = 0; i < 8; i++) consts[i] = c[i];
}

// head[]: src_words, table_words, dst_words, field_bits, largest, window_words, windows, image_words, block, grid, lds_bytes, moved,
// the number of entries of need
// dst_col[]: 64 x table_words values, live[]: table_words, sizes[]: num_groups, need[]: 64 x round_up(dst_words, 2); nothing is
// written beyond the capacities (all four NULL: the head alone); returns 0 when all were large enough.  window_words 0: the
// planner's own.  min_members NULL: no need table.
int consensus_host_plan(uint64_t num_cols, const uint32_t *group_of, uint64_t num_groups, const uint32_t *min_members, uint64_t num_rows,
                        uint64_t window_words, uint64_t *head, uint32_t *dst_col, uint64_t col_capacity, uint64_t *live, uint64_t live_capacity,
                        uint32_t *sizes, uint64_t sizes_capacity, uint32_t *need, uint64_t need_capacity)
{
    const bigsi::ConsensusPlan p = bigsi::plan_consensus_columns(num_cols, group_of, num_groups, min_members, num_rows, window_words);
    const uint64_t hd[13] = {p.src_words, p.table_words, p.dst_words, p.field_bits, p.largest,   p.window_words, p.windows,
                             p.image_words, p.block,     p.grid,      p.lds_bytes,  p.moved,     p.need.size()};
    for (int i = 0; i < 13; i++) head[i] = hd[i];
    if (p.dst_col.size() != p.table_words * 64 || p.live.size() != p.table_words || p.sizes.size() != num_groups) return 2;
    if (min_members && p.need.size() != round_up(p.dst_words, 2) * 64) return 2;
    if (!dst_col && !live && !sizes && !need) return 0;
    if (p.dst_col.size() > col_capacity || p.live.size() > live_capacity || p.sizes.size() > sizes_capacity || p.need.size() > need_capacity) return 1;
    for (uint64_t i = 0; i < p.dst_col.size(); i++) dst_col[i] = p.dst_col[i];
    for (uint64_t i = 0; i < p.live.size(); i++) live[i] = p.live[i];
    for (uint64_t i = 0; i < p.sizes.size(); i++) sizes[i] = p.sizes[i];
    for (uint64_t i = 0; i < p.need.size(); i++) need[i] = p.need[i];
    return 0;
}

// window j of a plan of dst_words destination words at window_words words per window: destination words [*first, *first + *count)
void consensus_host_window(uint64_t dst_words, uint64_t window_words, uint64_t j, uint64_t *first, uint64_t *count)
{
    bigsi::ConsensusPlan p;
    p.dst_words = dst_words;
    p.window_words = window_words;
    bigsi::consensus_window(p, j, first, count);
}

uint32_t consensus_host_field_bits(uint64_t largest) { return bigsi::consensus_field_bits(largest); }

uint64_t consensus_host_first_zero(const uint32_t *min_members, uint64_t num_groups) { return bigsi::consensus_first_zero(min_members, num_groups); }

}
