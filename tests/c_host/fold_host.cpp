// CPU pin of plan_fold_rows (bigsi_amd/csrc/bigsi_launch.hpp): the launch shape of the row folding -- column segments x blocks of
// destination rows, and the rows a lane folds per step -- compiled here as plain host C++.  tests/test_fold_rows_host.py loads it and
// checks the cover, the grid size and the kernel's register-budget invariant.
// Test infrastructure only: nothing in the product loads this file.
#include "../../bigsi_amd/csrc/bigsi_launch.hpp"

extern "C" {

// out[]: block, seg_groups, rows_per_step, rows_per_block, row_blocks, grid, kFoldLoads, kFoldMaxLoads, kFoldWaves, kFoldMinRows
void fold_host_plan(uint64_t m_dst, uint64_t factor, uint64_t stride_words, uint64_t *out)
{
    const bigsi::FoldPlan p = bigsi::plan_fold_rows(m_dst, factor, stride_words);
    const uint64_t v[10] = {p.block, p.seg_groups, p.rows_per_step, p.rows_per_block, p.row_blocks, p.grid, (uint64_t)bigsi::kFoldLoads,
                            (uint64_t)bigsi::kFoldMaxLoads, bigsi::kFoldWaves, bigsi::kFoldMinRows};
    for (int i = 0; i < 10; i++) out[i] = v[i];
}

}
