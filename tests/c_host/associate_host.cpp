// CPU pin of plan_associate (bigsi_amd/csrc/bigsi_launch.hpp): the launch shape of the group association's two kernels, compiled here
// as plain host C++.  tests/test_associate_host.py loads it and checks it against a plain Python restatement (tests/associate_ref.py).
// Test infrastructure only: nothing in the product loads this file.
#include "../../bigsi_amd/csrc/bigsi_launch.hpp"

extern "C" {

// out[]: kBlock, kAssociateMaxGroups, kAssociateNoGroup, kClassifyNoGroup, kAssociateQueries, kAssociateGroupBlock, kTallyChunkSeqs
void associate_host_constants(uint64_t *out)
{
    const uint64_t v[7] = {(uint64_t)bigsi::kBlock,          bigsi::kAssociateMaxGroups,  bigsi::kAssociateNoGroup, bigsi::kClassifyNoGroup,
                           bigsi::kAssociateQueries, bigsi::kAssociateGroupBlock, bigsi::kTallyChunkSeqs};
    for (int i = 0; i < 7; i++) out[i] = v[i];
}

// out[]: block, grid, mask_grid, lds_bytes, passes, mask_bytes, too_large, bad_groups
void associate_host_plan(uint64_t n_seqs, uint64_t wv, uint64_t n_groups, uint64_t *out)
{
    const bigsi::AssociatePlan p = bigsi::plan_associate(n_seqs, wv, n_groups);
    const uint64_t v[8] = {p.block, p.grid, p.mask_grid, p.lds_bytes, p.passes, p.mask_bytes, p.too_large, p.bad_groups ? 1u : 0u};
    for (int i = 0; i < 8; i++) out[i] = v[i];
}

}
