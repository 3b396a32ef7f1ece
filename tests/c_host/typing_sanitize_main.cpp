// A stand-alone program (its own main) that drives the host side of the locus typing -- plan_typing, the key function typing_key and
// the label validation typing_bad_label (bigsi_amd/csrc/bigsi_launch.hpp) -- and the CPU twin's bigsi_cpu_typing
// (bigsi_amd/cpu/bigsi_cpu.cpp) over the refused arguments and odd shapes at the width edges, checks the planner's invariants, the key
// against 128-bit arithmetic and the twin against the twin's own per-sequence search, and is meant to be built with
// -fsanitize=address,undefined and run on the CPU: tests/test_typing_host.py compiles it together with bigsi_cpu.cpp and runs it.
// Nothing sanitized is loaded into Python.  Test infrastructure only: nothing in the product loads this file.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../bigsi_amd/csrc/bigsi_launch.hpp"
#include "bigsi_cpu_typing.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            fprintf(stderr, "FAILED %s: ", #cond);        \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
            exit(1);                                      \
        }                                                 \
    } while (0)

static void planner()
{
    const uint64_t T = bigsi::kTypingTile, W = (uint64_t)bigsi::kBlock / 64;
    for (uint64_t n : {0ull, 1ull, 63ull, 64ull, 65ull, 4096ull, 64ull * 0x7FFFFFFFull, 64ull * 0x7FFFFFFFull + 1, 0xFFFFFFFFFFull})
        for (uint64_t wv : {1ull, 3ull, 4ull, 5ull, 13ull, 15625ull, 4ull * 0x7FFFFFFFull, 4ull * 0x7FFFFFFFull + 1, 1ull << 34, 1ull << 62, ~0ull})
            for (uint64_t l : {0ull, 1ull, 3ull, 4ull, 5ull, 357ull, 358ull, 1ull << 20, (1ull << 20) + 1, 1ull << 40}) {
                const bigsi::TypingPlan p = bigsi::plan_typing(n, wv, l);
                CHECK(p.block == (uint32_t)bigsi::kBlock && p.tile == T && p.tiles * T >= n && (p.tiles == 0 || (p.tiles - 1) * T < n), "%llu records", (unsigned long long)n);
                CHECK((unsigned __int128)p.word_groups * W >= wv && (p.word_groups - 1) * W < wv && p.words_grid == p.word_groups, "%llu words", (unsigned long long)wv);
                const unsigned __int128 product = (unsigned __int128)p.word_groups * p.tiles;
                CHECK(p.grid == (product > ~0ull ? ~0ull : (uint64_t)product), "grid");
                CHECK(p.bad_loci == (l == 0 || l > bigsi::kTypingMaxLoci), "%llu loci", (unsigned long long)l);
                if (p.bad_loci) {
                    CHECK((p.too_large != 0) == (p.grid > 0x7FFFFFFFull || p.words_grid > 0x7FFFFFFFull) && p.counts_grid == 0 && p.cell_bytes == 0, "too_large without loci");
                    continue;
                }
                CHECK(p.loci_grid * W >= l && (p.loci_grid - 1) * W < l && p.counts_grid == p.loci_grid + p.words_grid, "counts grid");
                CHECK((p.too_large != 0) == (p.grid > 0x7FFFFFFFull || p.counts_grid > 0x7FFFFFFFull), "too_large");
                CHECK(p.too_many_bytes == ((unsigned __int128)768 * l * wv > bigsi::kTypingCellBytes), "the cell limit");
                CHECK(p.cell_bytes == (p.too_many_bytes ? 0 : 768 * l * wv), "cell bytes");
            }
    CHECK(BIGSI_TYPING_NONE == bigsi::kTypingNone && BIGSI_TYPING_MAX_ALLELE == bigsi::kTypingMaxAllele && BIGSI_TYPING_MAX_LOCI == bigsi::kTypingMaxLoci &&
              BIGSI_TYPING_CELL_BYTES == bigsi::kTypingCellBytes,
          "constants");
}

static void keys()
{
    const uint32_t us[] = {1u, 2u, 3u, 64u, 65535u, 65536u, 1u << 20, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    const uint32_t alleles[] = {0u, 1u, 0x7FFFFFFFu, 0xFFFFFFFEu};
    for (uint32_t u : us)
        for (uint32_t c : {0u, 1u, u / 2, u - 1, u})
            for (uint32_t a : alleles) {
                if (c > u) continue;
                const uint64_t key = bigsi::typing_key(c, u, a);
                const unsigned __int128 score = (unsigned __int128)c * 0xFFFFFFFFull / u;
                CHECK(key >> 32 == (uint64_t)score && (uint32_t)key == 0xFFFFFFFFu - a && key != 0, "key of %u / %u, allele %u", c, u, a);
                CHECK((c == u) == (key >> 32 == 0xFFFFFFFFull), "only a whole record scores 2^32 - 1 (%u / %u)", c, u);
            }
    for (int i = 0; i < 200000; i++) {
        const uint32_t u = (uint32_t)(rnd() >> (rnd() % 32)) | 1u, c = (uint32_t)(rnd() % ((uint64_t)u + 1)), a = (uint32_t)rnd() % 0xFFFFFFFFu;
        const unsigned __int128 score = (unsigned __int128)c * 0xFFFFFFFFull / u;
        CHECK(bigsi::typing_key(c, u, a) == ((uint64_t)score << 32 | (0xFFFFFFFFu - a)), "random key %u / %u", c, u);
    }
    // the higher fraction has the higher key whatever the identities; equal fractions: the lower identity
    CHECK(bigsi::typing_key(2, 3, 0xFFFFFFFEu) > bigsi::typing_key(1, 2, 0) && bigsi::typing_key(1, 2, 7) > bigsi::typing_key(2, 4, 8), "order");
}

static void labels()
{
    std::vector<uint32_t> lo(130, 0), al(130, 5);
    CHECK(bigsi::typing_bad_label(lo.data(), al.data(), lo.size(), 1) == lo.size(), "all zero");
    lo[129] = 1;
    CHECK(bigsi::typing_bad_label(lo.data(), al.data(), lo.size(), 1) == 129 && bigsi::typing_bad_label(lo.data(), al.data(), lo.size(), 2) == lo.size(), "the last record");
    lo[129] = BIGSI_TYPING_NONE;
    al[129] = 0xFFFFFFFFu;
    CHECK(bigsi::typing_bad_label(lo.data(), al.data(), lo.size(), 1) == lo.size(), "a record without a locus: its allele is not looked at");
    al[64] = 0xFFFFFFFFu;
    CHECK(bigsi::typing_bad_label(lo.data(), al.data(), lo.size(), 1) == 64, "an identity above BIGSI_TYPING_MAX_ALLELE");
    al[64] = BIGSI_TYPING_MAX_ALLELE;
    CHECK(bigsi::typing_bad_label(lo.data(), al.data(), lo.size(), 1) == lo.size() && bigsi::typing_bad_label(lo.data(), al.data(), 0, 1) == 0, "the largest identity");
}

static bool bit(const uint8_t *row, uint64_t c) { return (row[c >> 3] >> (7 - (c & 7))) & 1u; }

static void twin(uint64_t m, uint64_t n_cols, uint32_t h, uint32_t k, uint64_t n_seqs, double threshold, uint32_t n_loci, bool masked)
{
    bigsi_cpu_index *ix = nullptr;
    CHECK(bigsi_cpu_open(m, n_cols, n_cols, h, 0, &ix) == 0, "%s", bigsi_cpu_last_error());
    bigsi_hip_info inf;
    CHECK(bigsi_cpu_get_info(ix, &inf) == 0, "%s", bigsi_cpu_last_error());
    const uint64_t stride = inf.row_stride_bytes, rb = (n_cols + 7) / 8, cells = n_loci * n_cols;
    std::vector<uint8_t> rows(m * stride);
    for (auto &b : rows) b = (uint8_t)(rnd() | rnd());          // dense rows, junk behind num_cols included: hits at every threshold
    std::vector<uint64_t> ids(m);
    for (uint64_t r = 0; r < m; r++) ids[r] = r;
    CHECK(bigsi_cpu_set_rows(ix, ids.data(), m, rows.data(), stride) == 0, "%s", bigsi_cpu_last_error());
    std::string blob;
    std::vector<uint64_t> off(n_seqs + 1, 0);
    for (uint64_t i = 0; i < n_seqs; i++) {
        const uint64_t len = i == 1 ? k - 1 : k + rnd() % 9;
        for (uint64_t j = 0; j < len; j++) blob.push_back("ACGT"[rnd() & 3]);
        off[i + 1] = blob.size();
    }
    std::vector<uint32_t> locus_of(n_seqs), allele_of(n_seqs);
    for (uint64_t i = 0; i < n_seqs; i++) {
        locus_of[i] = rnd() % 5 == 0 ? BIGSI_TYPING_NONE : (uint32_t)(rnd() % n_loci);
        allele_of[i] = locus_of[i] == BIGSI_TYPING_NONE ? 0xFFFFFFFFu : (uint32_t)(n_seqs - i);      // (later records: lower identities)
    }
    std::vector<uint8_t> columns(rb);
    for (auto &b : columns) b = (uint8_t)(rnd() | rnd());       // (junk behind num_cols included)
    const uint8_t *cols = masked ? columns.data() : nullptr;
    auto selected = [&](uint64_t c) { return !cols || bit(cols, c); };
    std::vector<uint64_t> best(cells + 1, 0xABABABABABABABABull);
    std::vector<uint32_t> hits(cells + 1, 0xABABABABu), lc((n_loci + 1) * 3, 0xABABABABu), sc((n_cols + 1) * 2, 0xABABABABu), rec(n_loci + 1, 0xABABABABu);
    auto call = [&](double t, const uint32_t *lo, const uint32_t *al, uint32_t nl, uint64_t ccap, uint64_t scap, uint32_t *l) {
        return bigsi_cpu_typing(ix, blob.data(), off.data(), n_seqs, k, t, lo, al, nl, cols, best.data(), hits.data(), ccap, l, sc.data(), scap, rec.data());
    };
    const uint32_t *lo = locus_of.data(), *al = allele_of.data();
    CHECK(call(1.5, lo, al, n_loci, cells, n_cols, lc.data()) == BIGSI_ERR_INVALID, "threshold 1.5");
    CHECK(call(threshold, nullptr, al, n_loci, cells, n_cols, lc.data()) == BIGSI_ERR_INVALID, "NULL locus_of");
    CHECK(call(threshold, lo, nullptr, n_loci, cells, n_cols, lc.data()) == BIGSI_ERR_INVALID, "NULL allele_of");
    CHECK(call(threshold, lo, al, n_loci, cells, n_cols, nullptr) == BIGSI_ERR_INVALID, "NULL locus_counts");
    CHECK(call(threshold, lo, al, 0, cells, n_cols, lc.data()) == BIGSI_ERR_INVALID, "no loci");
    CHECK(call(threshold, lo, al, BIGSI_TYPING_MAX_LOCI + 1, cells, n_cols, lc.data()) == BIGSI_ERR_INVALID && strstr(bigsi_cpu_last_error(), "BIGSI_TYPING_MAX_LOCI"), "too many loci");
    CHECK(call(threshold, lo, al, n_loci, cells - 1, n_cols, lc.data()) == BIGSI_ERR_CAPACITY, "cell capacity");
    CHECK(call(threshold, lo, al, n_loci, cells, n_cols - 1, lc.data()) == BIGSI_ERR_CAPACITY, "sample capacity");
    {
        std::vector<uint32_t> bad(locus_of);
        bad[n_seqs - 1] = n_loci;
        CHECK(call(threshold, bad.data(), al, n_loci, cells, n_cols, lc.data()) == BIGSI_ERR_INVALID && strstr(bigsi_cpu_last_error(), "locus_of["), "a locus of n_loci");
        bad = allele_of;
        std::vector<uint32_t> with_locus(locus_of);
        with_locus[n_seqs - 1] = 0;
        bad[n_seqs - 1] = 0xFFFFFFFFu;
        CHECK(call(threshold, with_locus.data(), bad.data(), n_loci, cells, n_cols, lc.data()) == BIGSI_ERR_INVALID && strstr(bigsi_cpu_last_error(), "allele_of["), "an identity of 2^32 - 1");
    }
    CHECK(best[0] == 0xABABABABABABABABull && hits[0] == 0xABABABABu && lc[0] == 0xABABABABu && sc[0] == 0xABABABABu && rec[0] == 0xABABABABu, "a refused call wrote its output");
    CHECK(call(threshold, lo, al, n_loci, cells, n_cols, lc.data()) == 0, "%s", bigsi_cpu_last_error());
    CHECK(best[cells] == 0xABABABABABABABABull && hits[cells] == 0xABABABABu, "wrote behind the cells");
    CHECK(lc[n_loci * 3] == 0xABABABABu && sc[n_cols * 2] == 0xABABABABu && rec[n_loci] == 0xABABABABu, "wrote behind the counts");
    // against the twin's own search, record by record, and typing_key
    std::vector<uint64_t> want(cells, 0);
    std::vector<uint32_t> nh(cells, 0), used(n_loci, 0);
    for (uint64_t i = 0; i < n_seqs; i++) {
        uint32_t nk, nu, mk;
        std::vector<uint64_t> hoff(2);
        std::vector<uint32_t> col(n_cols), cnt(n_cols);
        const uint64_t one[2] = {off[i], off[i + 1]};
        CHECK(bigsi_cpu_search_batch(ix, blob.data(), one, 1, k, threshold < 0 ? 0.0 : threshold, 0, &nk, &nu, &mk, hoff.data(), col.data(), cnt.data(), n_cols) == 0, "%s",
              bigsi_cpu_last_error());
        if (nu == 0 || locus_of[i] == BIGSI_TYPING_NONE) continue;
        used[locus_of[i]]++;
        if (threshold <= 0.0) CHECK(hoff[1] == n_cols, "at threshold 0 every column is a hit");
        for (uint64_t j = 0; j < hoff[1]; j++) {
            if (!selected(col[j])) continue;
            const uint64_t cell = locus_of[i] * n_cols + col[j], key = bigsi::typing_key(cnt[j], nu, allele_of[i]);
            if (key > want[cell]) want[cell] = key;
            nh[cell]++;
        }
    }
    CHECK(memcmp(best.data(), want.data(), cells * 8) == 0 && memcmp(hits.data(), nh.data(), cells * 4) == 0, "the cells at %llu columns", (unsigned long long)n_cols);
    CHECK(memcmp(rec.data(), used.data(), n_loci * 4) == 0, "records");
    std::vector<uint32_t> called(n_cols, 0), exact(n_cols, 0);
    for (uint32_t l = 0; l < n_loci; l++) {
        uint32_t n[3] = {0, 0, 0};
        for (uint64_t c = 0; c < n_cols; c++) {
            const uint64_t b = want[l * n_cols + c];
            CHECK(selected(c) || (b == 0 && nh[l * n_cols + c] == 0), "an unselected column holds a cell");
            CHECK((b != 0) == (nh[l * n_cols + c] != 0), "a key without a hit");
            n[0] += b != 0;
            n[1] += b >> 32 == 0xFFFFFFFFull;
            n[2] += nh[l * n_cols + c] > 1;
            called[c] += b != 0;
            exact[c] += b >> 32 == 0xFFFFFFFFull;
        }
        CHECK(memcmp(&lc[l * 3], n, sizeof n) == 0, "the counts of locus %u", l);
    }
    for (uint64_t c = 0; c < n_cols; c++) CHECK(sc[c * 2] == called[c] && sc[c * 2 + 1] == exact[c], "the counts of column %llu", (unsigned long long)c);
    // without cells: the same counts
    std::vector<uint32_t> lc2(n_loci * 3), sc2(n_cols * 2), rec2(n_loci);
    CHECK(bigsi_cpu_typing(ix, blob.data(), off.data(), n_seqs, k, threshold, lo, al, n_loci, cols, nullptr, nullptr, 0, lc2.data(), sc2.data(), n_cols, rec2.data()) == 0, "%s",
          bigsi_cpu_last_error());
    CHECK(memcmp(lc2.data(), lc.data(), lc2.size() * 4) == 0 && memcmp(sc2.data(), sc.data(), sc2.size() * 4) == 0 && memcmp(rec2.data(), rec.data(), rec2.size() * 4) == 0, "NULL cells");
    CHECK(bigsi_cpu_close(ix) == 0, "%s", bigsi_cpu_last_error());
}

int main()
{
    planner();
    keys();
    labels();
    for (uint64_t n_cols : {1ull, 63ull, 64ull, 65ull, 127ull, 129ull, 200ull})
        for (double t : {1.0, 0.5, 0.0, -1.0})
            for (uint64_t n_seqs : {1ull, 2ull, 9ull})
                for (uint32_t n_loci : {1u, 3u, 65u})
                    for (bool masked : {false, true}) twin(97, n_cols, 2, 5, n_seqs, t, n_loci, masked);
    printf("typing planner, key and twin: ok\n");
    return 0;
}
