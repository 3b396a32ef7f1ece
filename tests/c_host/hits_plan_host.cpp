// CPU pin of the hit-list compaction's launch rule and of the export's size in bigsi_amd/csrc/bigsi_launch.hpp (plan_hits,
// export_spec), compiled here as plain host C++.  tests/test_hits_plan_host.py loads it, pins the constants and the shapes the header
// states and checks the invariants over a seeded sweep; tests/test_hits_cases_host.py asks it which path every case of
// tests/hits_cases.py takes.
// Test infrastructure only: nothing in the product loads this file.
#include "../../bigsi_amd/csrc/bigsi_launch.hpp"

extern "C" {

// out[]: items per group, groups, single-workgroup body
void hits_host_plan(uint64_t nchunks, uint32_t n_shards, uint64_t *out)
{
    const bigsi::HitsPlan p = bigsi::plan_hits(nchunks, n_shards);
    out[0] = p.ipb;
    out[1] = p.groups;
    out[2] = p.single;
}

uint64_t hits_host_export_spec(uint64_t n_seqs, uint64_t capacity) { return bigsi::export_spec(n_seqs, capacity); }

// the shipped constants: most groups, most items of the one-group launch, entries the lists start with, the export's floor, its
// share per sequence, its ceiling, threads of a workgroup (= words of an item)
void hits_host_constants(uint64_t *out)
{
    out[0] = bigsi::kHitsMaxGroups;
    out[1] = bigsi::kHitsOneGroupItems;
    out[2] = bigsi::kHitsInitialCapacity;
    out[3] = bigsi::kExportSpecMin;
    out[4] = bigsi::kExportSpecPerSeq;
    out[5] = bigsi::kExportSpecMax;
    out[6] = bigsi::kBlock;
}

}
