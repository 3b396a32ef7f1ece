// CPU pin of plan_genotype and genotype_bad_allele (bigsi_amd/csrc/bigsi_launch.hpp): the launch shapes of the panel genotyping's three
// kernels and the allele_of validation, compiled here as plain host C++.  tests/test_genotype_host.py loads it and checks it against a
// plain Python restatement (tests/genotype_ref.py).  Test infrastructure only: nothing in the product loads this file.
#include "../../bigsi_amd/csrc/bigsi_launch.hpp"

extern "C" {

// out[]: kBlock, kGenotypeNone, kGenotypeMaxVariants, kGenotypePlaneBytes, kGenotypeTile, kGenotypeLoads, kTallyChunkSeqs
void genotype_host_constants(uint64_t *out)
{
    const uint64_t v[7] = {(uint64_t)bigsi::kBlock,    bigsi::kGenotypeNone,  bigsi::kGenotypeMaxVariants, bigsi::kGenotypePlaneBytes,
                           bigsi::kGenotypeTile, bigsi::kGenotypeLoads, bigsi::kTallyChunkSeqs};
    for (int i = 0; i < 7; i++) out[i] = v[i];
}

// out[]: block, tile, word_blocks, tiles, grid, variants_grid, samples_grid, plane_bytes, too_large, bad_variants, too_many_bytes
void genotype_host_plan(uint64_t n_seqs, uint64_t wv, uint64_t n_variants, uint64_t *out)
{
    const bigsi::GenotypePlan p = bigsi::plan_genotype(n_seqs, wv, n_variants);
    const uint64_t v[11] = {p.block, p.tile, p.word_blocks, p.tiles, p.grid, p.variants_grid, p.samples_grid, p.plane_bytes, p.too_large,
                            p.bad_variants ? 1u : 0u, p.too_many_bytes ? 1u : 0u};
    for (int i = 0; i < 11; i++) out[i] = v[i];
}

uint64_t genotype_host_bad_allele(const uint32_t *allele_of, uint64_t n_entries, uint64_t n_variants)
{
    return bigsi::genotype_bad_allele(allele_of, n_entries, n_variants);
}

}
