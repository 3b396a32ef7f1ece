// CPU pin of plan_pairwise and pairwise_tables (bigsi_amd/csrc/bigsi_launch.hpp): the chunks, slices, tiles and scratch of the
// pairwise popcounts and the per-call tables, compiled here as plain host C++, and a replay of what the three kernels do with them
// (planes by ballot order, 32-bit partial counts per tile and slice, the sum through the maps and the mirror tile) on rows in host
// memory.  tests/test_pairwise_host.py loads it and checks plan invariants and the replay against numpy;
// tests/test_gpu_pairwise.py reads the chunk and slice boundaries from it.
// Test infrastructure only: nothing in the product loads this file.
#include <string.h>

#include "../../bigsi_amd/csrc/bigsi_launch.hpp"

extern "C" {

// consts[]: kPairwiseMaxPairs, kPairTile, kPairStageWords, kPairPlaneBytes, kPairPartialBytes, kPairMaxChunkWords, kPairSplitWords,
// kPairMinSliceWords, kPairWantGroups
void pairwise_host_constants(uint64_t *consts)
{
    const uint64_t c[9] = {bigsi::kPairwiseMaxPairs,  (uint64_t)bigsi::kPairTile, (uint64_t)bigsi::kPairStageWords, bigsi::kPairPlaneBytes, bigsi::kPairPartialBytes,
                           bigsi::kPairMaxChunkWords, bigsi::kPairSplitWords,     bigsi::kPairMinSliceWords,        bigsi::kPairWantGroups};
    for (int i = 0; i < 9; i++) consts[i] = c[i];
}

// head[]: total_words, chunk_words, chunks, slice_words, slices, tiles_i, tiles_j, tiles, plane_bytes, partial_bytes
void pairwise_host_plan(uint64_t na_unique, uint64_t nb_unique, int symmetric, uint64_t num_rows, uint64_t stride_words, uint64_t *head)
{
    const bigsi::PairwisePlan p = bigsi::plan_pairwise(na_unique, nb_unique, symmetric != 0, num_rows, stride_words);
    const uint64_t hd[10] = {p.total_words, p.chunk_words, p.chunks, p.slice_words, p.slices, p.tiles_i, p.tiles_j, p.tiles, p.plane_bytes, p.partial_bytes};
    for (int i = 0; i < 10; i++) head[i] = hd[i];
}

// words of chunk c and its slices, as the entry point asks for them
void pairwise_host_chunk(uint64_t na_unique, uint64_t nb_unique, int symmetric, uint64_t num_rows, uint64_t stride_words, uint64_t c, uint64_t *words, uint64_t *slices)
{
    const bigsi::PairwisePlan p = bigsi::plan_pairwise(na_unique, nb_unique, symmetric != 0, num_rows, stride_words);
    *words = bigsi::pairwise_chunk_words(p, c);
    *slices = bigsi::pairwise_chunk_slices(p, *words);
}

uint64_t pairwise_host_first_bad(const uint32_t *cols, uint64_t n, uint64_t num_cols) { return bigsi::pairwise_first_bad(cols, n, num_cols); }

// sizes[]: distinct columns (planes), distinct words, distinct A, distinct B (0: symmetric)
void pairwise_host_table_sizes(const uint32_t *cols_a, uint64_t na, const uint32_t *cols_b, uint64_t nb, uint64_t *sizes)
{
    const bigsi::PairwiseTables t = bigsi::pairwise_tables(cols_a, na, cols_b, nb);
    sizes[0] = t.bit.size(); sizes[1] = t.words.size(); sizes[2] = t.plane_a.size(); sizes[3] = t.plane_b.size();
}

// The three kernels on the host.  rows: alloc_rows x stride_bytes bytes in the row format, of which num_rows count (the rest is what
// an in-place fold leaves behind); cols_b == NULL: symmetric.  out: na x nb.  Returns 0, or a positive code when an invariant the
// kernels rely on does not hold (1: a 32-bit counter would wrap, 2: a slice or chunk is empty or the rows are not covered once,
// 3: a table is inconsistent).
int pairwise_host_replay(const uint8_t *rows, uint64_t num_rows, uint64_t stride_bytes, const uint32_t *cols_a, uint64_t na, const uint32_t *cols_b, uint64_t nb,
                         uint64_t *out)
{
    const bool symmetric = cols_b == nullptr;
    if (symmetric) nb = na;
    const bigsi::PairwiseTables t = bigsi::pairwise_tables(cols_a, na, cols_b, nb);
    const uint64_t nua = t.plane_a.size(), nub = symmetric ? nua : t.plane_b.size(), distinct = t.bit.size();
    const std::vector<uint32_t> &plane_b = symmetric ? t.plane_a : t.plane_b, &map_b = symmetric ? t.map_a : t.map_b;
    if (t.first.size() != t.words.size() + 1 || t.first.back() != distinct || t.map_a.size() != na || map_b.size() != nb) return 3;
    const bigsi::PairwisePlan p = bigsi::plan_pairwise(nua, nub, symmetric, num_rows, stride_bytes / 8);
    if (distinct * p.chunk_words * 8 > p.plane_bytes) return 3;
    std::vector<uint64_t> planes(distinct * p.chunk_words), seen(p.total_words, 0);
    std::vector<uint32_t> partial(p.slices * nua * nub);
    const uint32_t T = bigsi::kPairTile;
    for (uint64_t c = 0; c < p.chunks; c++) {
        const uint64_t words = bigsi::pairwise_chunk_words(p, c), slices = bigsi::pairwise_chunk_slices(p, words), row0 = c * p.chunk_words * 64;
        if (words == 0 || slices == 0 || slices > p.slices) return 2;
        // k_columns_to_planes: group g, lane k = row row0 + 64 g + k; the column's bit as it lies in the little-endian 64-bit word
        for (uint64_t g = 0; g < words; g++)
            for (uint64_t k = 0; k < t.words.size(); k++)
                for (uint32_t u = t.first[k]; u < t.first[k + 1]; u++) {
                    uint64_t word = 0;
                    for (uint64_t lane = 0; lane < 64; lane++) {
                        const uint64_t r = row0 + g * 64 + lane;
                        if (r >= num_rows) continue;
                        uint64_t v;
                        memcpy(&v, rows + r * stride_bytes + (uint64_t)t.words[k] * 8, 8);          // (little-endian hosts, as the device)
                        word |= ((v >> t.bit[u]) & 1ull) << lane;
                    }
                    planes[(uint64_t)u * p.chunk_words + g] = word;
                }
        // k_pair_popcount: tile (ti, tj) x slice s; symmetric calls leave the tiles below the diagonal alone
        std::fill(partial.begin(), partial.end(), 0xDEADBEEFu);
        for (uint64_t s = 0; s < slices; s++) {
            const uint64_t w_begin = s * p.slice_words, w_end = std::min(w_begin + p.slice_words, words);
            if (w_begin >= w_end) return 2;
            if ((w_end - w_begin) * 64 > 0xFFFFFFFFull) return 1;
            for (uint64_t w = w_begin; w < w_end; w++) seen[c * p.chunk_words + w]++;
            for (uint64_t ia = 0; ia < nua; ia++)
                for (uint64_t ib = 0; ib < nub; ib++) {
                    if (symmetric && ib / T < ia / T) continue;
                    uint32_t acc = 0;
                    for (uint64_t w = w_begin; w < w_end; w++)
                        acc += (uint32_t)__builtin_popcountll(planes[(uint64_t)t.plane_a[ia] * p.chunk_words + w] & planes[(uint64_t)plane_b[ib] * p.chunk_words + w]);
                    partial[(s * nua + ia) * nub + ib] = acc;
                }
        }
        // k_pair_popcount_sum
        for (uint64_t e = 0; e < na * nb; e++) {
            uint32_t u = t.map_a[e / nb], v = map_b[e % nb];
            if (symmetric && v / T < u / T) std::swap(u, v);
            uint64_t sum = 0;
            for (uint64_t s = 0; s < slices; s++) sum += partial[(s * nua + u) * nub + v];
            out[e] = c ? out[e] + sum : sum;
        }
    }
    for (uint64_t w = 0; w < p.total_words; w++)
        if (seen[w] != 1) return 2;
    return 0;
}

}
