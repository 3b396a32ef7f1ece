// CPU pin of plan_classify and classify_bad_column (bigsi_amd/csrc/bigsi_launch.hpp): the launch shape of the read classification's
// kernel and the validation of a caller's group_of, compiled here as plain host C++.  tests/test_classify_host.py loads it and checks
// both against a plain Python restatement (tests/classify_ref.py).
// Test infrastructure only: nothing in the product loads this file.
#include "../../bigsi_amd/csrc/bigsi_launch.hpp"

extern "C" {

// out[]: kBlock, kClassifyMaxGroups, kClassifyNoGroup
void classify_host_constants(uint64_t *out)
{
    const uint64_t v[3] = {(uint64_t)bigsi::kBlock, bigsi::kClassifyMaxGroups, bigsi::kClassifyNoGroup};
    for (int i = 0; i < 3; i++) out[i] = v[i];
}

// out[]: block, grid, table_bytes, lds_bytes, too_large, bad_groups
void classify_host_plan(uint64_t n_seqs, uint64_t wv, uint64_t n_groups, uint64_t *out)
{
    const bigsi::ClassifyPlan p = bigsi::plan_classify(n_seqs, wv, n_groups);
    const uint64_t v[6] = {p.block, p.grid, p.table_bytes, p.lds_bytes, p.too_large, p.bad_groups ? 1u : 0u};
    for (int i = 0; i < 6; i++) out[i] = v[i];
}

uint64_t classify_host_bad_column(const uint32_t *group_of, uint64_t n_entries, uint64_t n_groups)
{
    return bigsi::classify_bad_column(group_of, n_entries, n_groups);
}

}
