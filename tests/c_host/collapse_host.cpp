// CPU pin of plan_collapse_columns (bigsi_amd/csrc/bigsi_launch.hpp): the per-call tables of the column collapse -- dst_bit, the
// destination bit address of every source bit as it lies in memory, and live, the bits of every source word that move --, the launch
// shape and the destination window, compiled here as plain host C++.  tests/test_collapse_columns_host.py loads it and checks the
// tables against a bit-by-bit restatement of the row format and the window / LDS invariants over seeded shapes.
// Test infrastructure only: nothing in the product loads this file.
#include "../../bigsi_amd/csrc/bigsi_launch.hpp"

extern "C" {

// consts[]: kCollapseDropped, kCollapseWaves, kCollapseWindowWords, kCollapseLdsBytes, kCollapseLoads, kCollapseGathers, kBlock
void collapse_host_constants(uint64_t *consts)
{
    const uint64_t c[7] = {bigsi::kCollapseDropped, bigsi::kCollapseWaves,           bigsi::kCollapseWindowWords, bigsi::kCollapseLdsBytes,
                           (uint64_t)bigsi::kCollapseLoads, (uint64_t)bigsi::kCollapseGathers, (uint64_t)bigsi::kBlock};
    for (int i = 0; i < 7; i++) consts[i] = c[i];
}

// head[]: src_words, table_words, dst_words, window_words, windows, image_words, block, grid, lds_bytes, moved
// dst_bit[]: 64 x table_words values, live[]: table_words values; nothing is written beyond bit_capacity / live_capacity values (NULL
// tables: the head alone); returns 0 when both were large enough.  window_words 0: the planner's own.
int collapse_host_plan(uint64_t num_cols, const uint32_t *group_of, uint64_t num_groups, uint64_t num_rows, uint64_t window_words, uint64_t *head,
                       uint32_t *dst_bit, uint64_t bit_capacity, uint64_t *live, uint64_t live_capacity)
{
    const bigsi::CollapsePlan p = window_words ? bigsi::plan_collapse_columns(num_cols, group_of, num_groups, num_rows, window_words)
                                               : bigsi::plan_collapse_columns(num_cols, group_of, num_groups, num_rows);
    const uint64_t hd[10] = {p.src_words, p.table_words, p.dst_words, p.window_words, p.windows, p.image_words, p.block, p.grid, p.lds_bytes, p.moved};
    for (int i = 0; i < 10; i++) head[i] = hd[i];
    if (p.dst_bit.size() != p.table_words * 64 || p.live.size() != p.table_words) return 2;
    if (!dst_bit && !live) return 0;
    if (p.dst_bit.size() > bit_capacity || p.live.size() > live_capacity) return 1;
    for (uint64_t i = 0; i < p.dst_bit.size(); i++) dst_bit[i] = p.dst_bit[i];
    for (uint64_t i = 0; i < p.live.size(); i++) live[i] = p.live[i];
    return 0;
}

// window j of the plan of (num_groups, window_words; 0: the planner's own): destination words [*first, *first + *count)
void collapse_host_window(uint64_t num_groups, uint64_t window_words, uint64_t j, uint64_t *first, uint64_t *count)
{
    const bigsi::CollapsePlan p = window_words ? bigsi::plan_collapse_columns(0, nullptr, num_groups, 1, window_words)
                                               : bigsi::plan_collapse_columns(0, nullptr, num_groups, 1);
    bigsi::collapse_window(p, j, first, count);
}

uint64_t collapse_host_first_bad(uint64_t num_cols, const uint32_t *group_of, uint64_t num_groups)
{
    return bigsi::collapse_first_bad(num_cols, group_of, num_groups);
}

uint32_t collapse_host_mem_bit(uint32_t c) { return bigsi::collapse_mem_bit(c); }

}
