// CPU pin of plan_compact_columns (bigsi_amd/csrc/bigsi_launch.hpp): the per-call tables of the column compaction -- per source word
// its mask, the move masks of its compress network and the kept columns in front of it, per destination word the first source word
// that feeds it -- and the launch shape, compiled here as plain host C++.  tests/test_compact_columns_host.py loads it and checks the
// tables against a bit-by-bit restatement.
// Test infrastructure only: nothing in the product loads this file.
#include "../../bigsi_amd/csrc/bigsi_launch.hpp"

extern "C" {

// head[]: src_words, kept, dst_words, block, grid, kCompactRows
// words[]: 9 values per source word: mask, mv[0..5], before, count;  first_src[]: dst_words + 1 values.
// Nothing is written beyond words_capacity records / first_capacity values; returns 0 when both were large enough.
int compact_host_plan(uint64_t num_cols, const uint8_t *keep, uint64_t num_rows, uint64_t *head, uint64_t *words, uint64_t words_capacity,
                      uint64_t *first_src, uint64_t first_capacity)
{
    const bigsi::CompactPlan p = bigsi::plan_compact_columns(num_cols, keep, num_rows);
    const uint64_t hd[6] = {p.src_words, p.kept, p.dst_words, p.block, p.grid, (uint64_t)bigsi::kCompactRows};
    for (int i = 0; i < 6; i++) head[i] = hd[i];
    if (p.words.size() != p.src_words || p.first_src.size() != p.dst_words + 1) return 2;
    if (p.src_words > words_capacity || p.dst_words + 1 > first_capacity) return 1;
    for (uint64_t s = 0; s < p.src_words; s++) {
        const bigsi::CompactWord &w = p.words[s];
        uint64_t *o = words + 9 * s;
        o[0] = w.mask;
        for (int i = 0; i < 6; i++) o[1 + i] = w.mv[i];
        o[7] = w.before;
        o[8] = w.count;
    }
    for (uint64_t o = 0; o <= p.dst_words; o++) first_src[o] = p.first_src[o];
    return 0;
}

// K alone (what bigsi_hip_compact_columns asks before it builds any table)
uint64_t compact_host_count(uint64_t num_cols, const uint8_t *keep) { return bigsi::count_kept_columns(num_cols, keep); }

// the software pext the device runs on a word in plain column order: rec = one 9-value record of compact_host_plan
uint64_t compact_host_pext(uint64_t x, const uint64_t *rec)
{
    bigsi::CompactWord w{};
    w.mask = rec[0];
    for (int i = 0; i < 6; i++) w.mv[i] = rec[1 + i];
    return bigsi::compact_word(x, w);
}

}
