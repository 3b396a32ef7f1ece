// CPU pin of plan_kmer_prevalence (bigsi_amd/csrc/bigsi_launch.hpp): the launch shape of the k-mer prevalence sweep -- slices per
// k-mer, wavefronts that stride over the slots, loads in flight per step -- compiled here as plain host C++.
// tests/test_kmer_prevalence_host.py loads it and checks the cover, the grid size and the kernel's register-budget invariant.
// Test infrastructure only: nothing in the product loads this file.
#include "../../bigsi_amd/csrc/bigsi_launch.hpp"

extern "C" {

// out[]: block, segs, slices, segs_per_slice, waves_per_slice, waves, grid, segs_per_step, loads_per_step, partial_stride,
//        partial_entries, kPrevLoads, kPrevMaxLoads, kPrevWaves
void prevalence_host_plan(uint64_t total_pos, uint64_t total_unique, uint64_t wv, uint32_t h, uint64_t *out)
{
    const bigsi::PrevalencePlan p = bigsi::plan_kmer_prevalence(total_pos, total_unique, wv, h);
    const uint64_t v[14] = {p.block, p.segs, p.slices, p.segs_per_slice, p.waves_per_slice, p.waves, p.grid, p.segs_per_step, p.loads_per_step,
                            p.partial_stride, p.partial_entries, (uint64_t)bigsi::kPrevLoads, (uint64_t)bigsi::kPrevMaxLoads, bigsi::kPrevWaves};
    for (int i = 0; i < 14; i++) out[i] = v[i];
}

}
