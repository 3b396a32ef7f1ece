// CPU pin of plan_typing, typing_key and typing_bad_label (bigsi_amd/csrc/bigsi_launch.hpp): the launch shapes of the locus typing's two
// kernels, the key arithmetic k_locus_best compiles -- the one function, so this pin is the pin of the kernel's arithmetic -- and the
// label validation, compiled here as plain host C++.  tests/test_typing_host.py loads it and checks it against a plain Python
// restatement (tests/typing_ref.py).  Test infrastructure only: nothing in the product loads this file.
#include "../../bigsi_amd/csrc/bigsi_launch.hpp"

extern "C" {

// out[]: kBlock, kTypingNone, kTypingMaxAllele, kTypingMaxLoci, kTypingCellBytes, kTypingTile, kTypingLoads, kTallyChunkSeqs
void typing_host_constants(uint64_t *out)
{
    const uint64_t v[8] = {(uint64_t)bigsi::kBlock, bigsi::kTypingNone,  bigsi::kTypingMaxAllele, bigsi::kTypingMaxLoci,
                           bigsi::kTypingCellBytes, bigsi::kTypingTile, bigsi::kTypingLoads,     bigsi::kTallyChunkSeqs};
    for (int i = 0; i < 8; i++) out[i] = v[i];
}

// out[]: block, tile, word_groups, tiles, grid, loci_grid, words_grid, counts_grid, cell_bytes, too_large, bad_loci, too_many_bytes
void typing_host_plan(uint64_t n_seqs, uint64_t wv, uint64_t n_loci, uint64_t *out)
{
    const bigsi::TypingPlan p = bigsi::plan_typing(n_seqs, wv, n_loci);
    const uint64_t v[12] = {p.block,      p.tile,      p.word_groups,       p.tiles, p.grid, p.loci_grid, p.words_grid, p.counts_grid, p.cell_bytes,
                            p.too_large, p.bad_loci ? 1u : 0u, p.too_many_bytes ? 1u : 0u};
    for (int i = 0; i < 12; i++) out[i] = v[i];
}

uint64_t typing_host_key(uint32_t c, uint32_t u, uint32_t allele) { return bigsi::typing_key(c, u, allele); }

// keys of n (c, u, allele) triples at once
void typing_host_keys(const uint32_t *c, const uint32_t *u, const uint32_t *allele, uint64_t n, uint64_t *out)
{
    for (uint64_t i = 0; i < n; i++) out[i] = bigsi::typing_key(c[i], u[i], allele[i]);
}

uint64_t typing_host_bad_label(const uint32_t *locus_of, const uint32_t *allele_of, uint64_t n_entries, uint64_t n_loci)
{
    return bigsi::typing_bad_label(locus_of, allele_of, n_entries, n_loci);
}

}
