// A stand-alone program (its own main) that drives the host planner of the panel genotyping (plan_genotype and the allele_of validation
// genotype_bad_allele; bigsi_amd/csrc/bigsi_launch.hpp) and the CPU twin's bigsi_cpu_genotype (bigsi_amd/cpu/bigsi_cpu.cpp) over odd
// shapes at the width edges, checks the planner's invariants and the twin against the twin's own per-sequence search, and is meant to be
// built with -fsanitize=address,undefined and run on the CPU: tests/test_genotype_host.py compiles it together with bigsi_cpu.cpp and
// runs it.  Nothing sanitized is loaded into Python.  Test infrastructure only: nothing in the product loads this file.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../bigsi_amd/csrc/bigsi_launch.hpp"
#include "bigsi_cpu_genotype.h"

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
    const uint64_t T = bigsi::kGenotypeTile, B = (uint64_t)bigsi::kBlock;
    for (uint64_t n : {0ull, 1ull, 63ull, 64ull, 65ull, 4096ull, 64ull * 0x7FFFFFFFull, 64ull * 0x7FFFFFFFull + 1, 0xFFFFFFFFFFull})
        for (uint64_t wv : {1ull, 3ull, 4ull, 13ull, 255ull, 256ull, 257ull, 15625ull, 1ull << 26, 1ull << 34, 1ull << 62})
            for (uint64_t v : {0ull, 1ull, 3ull, 4ull, 5ull, 17179ull, 17180ull, 1ull << 20, (1ull << 20) + 1, 1ull << 40}) {
                const bigsi::GenotypePlan p = bigsi::plan_genotype(n, wv, v);
                CHECK(p.block == (uint32_t)bigsi::kBlock && p.tile == T && p.tiles * T >= n && (p.tiles == 0 || (p.tiles - 1) * T < n), "%llu probes", (unsigned long long)n);
                CHECK(p.word_blocks * B >= wv && (p.word_blocks - 1) * B < wv && p.samples_grid * 4 >= wv && (p.samples_grid - 1) * 4 < wv, "%llu words", (unsigned long long)wv);
                const unsigned __int128 product = (unsigned __int128)p.word_blocks * p.tiles;
                CHECK(p.grid == (product > ~0ull ? ~0ull : (uint64_t)product), "grid");
                CHECK((p.too_large != 0) == (p.grid > 0x7FFFFFFFull || p.samples_grid > 0x7FFFFFFFull), "too_large");
                CHECK(p.bad_variants == (v == 0 || v > bigsi::kGenotypeMaxVariants), "%llu variants", (unsigned long long)v);
                if (p.bad_variants) continue;
                CHECK(p.variants_grid * 4 >= v && (p.variants_grid - 1) * 4 < v, "variants grid");
                CHECK(p.too_many_bytes == ((unsigned __int128)16 * v * wv > bigsi::kGenotypePlaneBytes), "the plane limit");
                CHECK(p.plane_bytes == (p.too_many_bytes ? 0 : 16 * v * wv), "plane bytes");
            }
    std::vector<uint32_t> a(130, 0);
    CHECK(bigsi::genotype_bad_allele(a.data(), a.size(), 1) == a.size(), "all zero");
    a[129] = 2;
    CHECK(bigsi::genotype_bad_allele(a.data(), a.size(), 1) == 129 && bigsi::genotype_bad_allele(a.data(), a.size(), 2) == a.size(), "the last probe");
    a[129] = BIGSI_GENOTYPE_NONE;
    CHECK(bigsi::genotype_bad_allele(a.data(), a.size(), 1) == a.size(), "BIGSI_GENOTYPE_NONE is no allele");
    CHECK(BIGSI_GENOTYPE_NONE == bigsi::kGenotypeNone && BIGSI_GENOTYPE_MAX_VARIANTS == bigsi::kGenotypeMaxVariants && BIGSI_GENOTYPE_PLANE_BYTES == bigsi::kGenotypePlaneBytes,
          "constants");
}

static bool bit(const uint8_t *row, uint64_t c) { return (row[c >> 3] >> (7 - (c & 7))) & 1u; }

static void twin(uint64_t m, uint64_t n_cols, uint32_t h, uint32_t k, uint64_t n_seqs, double threshold, uint32_t n_variants, bool masked)
{
    bigsi_cpu_index *ix = nullptr;
    CHECK(bigsi_cpu_open(m, n_cols, n_cols, h, 0, &ix) == 0, "%s", bigsi_cpu_last_error());
    bigsi_hip_info inf;
    CHECK(bigsi_cpu_get_info(ix, &inf) == 0, "%s", bigsi_cpu_last_error());
    const uint64_t stride = inf.row_stride_bytes, rb = (n_cols + 7) / 8;
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
    std::vector<uint32_t> allele_of(n_seqs);
    for (uint64_t i = 0; i < n_seqs; i++) allele_of[i] = rnd() % 5 == 0 ? BIGSI_GENOTYPE_NONE : (uint32_t)(rnd() % (2 * n_variants));
    std::vector<uint8_t> columns(rb);
    for (auto &b : columns) b = (uint8_t)(rnd() | rnd());       // (junk behind num_cols included)
    const uint8_t *cols = masked ? columns.data() : nullptr;
    auto selected = [&](uint64_t c) { return !cols || bit(cols, c); };
    std::vector<uint8_t> ref((n_variants + 1) * rb, 0xAB), alt((n_variants + 1) * rb, 0xAB);
    std::vector<uint32_t> vc((n_variants + 1) * 4, 0xABABABABu), sc((n_cols + 1) * 2, 0xABABABABu), ap((n_variants + 1) * 2, 0xABABABABu);
    auto call = [&](double t, const uint32_t *al, uint32_t nv, uint64_t pcap, uint64_t scap, uint32_t *v) {
        return bigsi_cpu_genotype(ix, blob.data(), off.data(), n_seqs, k, t, al, nv, cols, ref.data(), alt.data(), pcap, v, sc.data(), scap, ap.data());
    };
    const uint64_t pcap = n_variants * rb;
    CHECK(call(1.5, allele_of.data(), n_variants, pcap, n_cols, vc.data()) == BIGSI_ERR_INVALID, "threshold 1.5");
    CHECK(call(threshold, nullptr, n_variants, pcap, n_cols, vc.data()) == BIGSI_ERR_INVALID, "NULL allele_of");
    CHECK(call(threshold, allele_of.data(), n_variants, pcap, n_cols, nullptr) == BIGSI_ERR_INVALID, "NULL variant_counts");
    CHECK(call(threshold, allele_of.data(), 0, pcap, n_cols, vc.data()) == BIGSI_ERR_INVALID, "no variants");
    CHECK(call(threshold, allele_of.data(), BIGSI_GENOTYPE_MAX_VARIANTS + 1, pcap, n_cols, vc.data()) == BIGSI_ERR_INVALID && strstr(bigsi_cpu_last_error(), "BIGSI_GENOTYPE_MAX_VARIANTS"),
          "too many variants");
    CHECK(call(threshold, allele_of.data(), n_variants, pcap - 1, n_cols, vc.data()) == BIGSI_ERR_CAPACITY, "plane capacity");
    CHECK(call(threshold, allele_of.data(), n_variants, pcap, n_cols - 1, vc.data()) == BIGSI_ERR_CAPACITY, "sample capacity");
    {
        std::vector<uint32_t> bad(allele_of);
        bad[n_seqs - 1] = 2 * n_variants;
        CHECK(call(threshold, bad.data(), n_variants, pcap, n_cols, vc.data()) == BIGSI_ERR_INVALID && strstr(bigsi_cpu_last_error(), "allele_of["), "an allele of 2 n_variants");
    }
    CHECK(ref[0] == 0xAB && alt[0] == 0xAB && vc[0] == 0xABABABABu && sc[0] == 0xABABABABu && ap[0] == 0xABABABABu, "a refused call wrote its output");
    CHECK(call(threshold, allele_of.data(), n_variants, pcap, n_cols, vc.data()) == 0, "%s", bigsi_cpu_last_error());
    for (uint64_t j = 0; j < rb; j++) CHECK(ref[n_variants * rb + j] == 0xAB && alt[n_variants * rb + j] == 0xAB, "wrote behind the planes");
    CHECK(vc[n_variants * 4] == 0xABABABABu && sc[n_cols * 2] == 0xABABABABu && ap[n_variants * 2] == 0xABABABABu, "wrote behind the counts");
    // against the twin's own search, probe by probe
    std::vector<uint8_t> want[2] = {std::vector<uint8_t>(n_variants * rb, 0), std::vector<uint8_t>(n_variants * rb, 0)};
    std::vector<uint32_t> used(n_variants * 2, 0);
    for (uint64_t i = 0; i < n_seqs; i++) {
        uint32_t nk, nu, mk;
        std::vector<uint64_t> hoff(2);
        std::vector<uint32_t> col(n_cols), cnt(n_cols);
        const uint64_t one[2] = {off[i], off[i + 1]};
        CHECK(bigsi_cpu_search_batch(ix, blob.data(), one, 1, k, threshold < 0 ? 0.0 : threshold, 0, &nk, &nu, &mk, hoff.data(), col.data(), cnt.data(), n_cols) == 0, "%s",
              bigsi_cpu_last_error());
        if (nu == 0 || allele_of[i] == BIGSI_GENOTYPE_NONE) continue;
        used[allele_of[i]]++;
        if (threshold <= 0.0) CHECK(hoff[1] == n_cols, "at threshold 0 every column is a hit");
        for (uint64_t j = 0; j < hoff[1]; j++)
            if (selected(col[j])) want[allele_of[i] & 1][(allele_of[i] >> 1) * rb + (col[j] >> 3)] |= (uint8_t)(0x80u >> (col[j] & 7));
    }
    CHECK(memcmp(ref.data(), want[0].data(), want[0].size()) == 0 && memcmp(alt.data(), want[1].data(), want[1].size()) == 0, "the planes at %llu columns", (unsigned long long)n_cols);
    CHECK(memcmp(ap.data(), used.data(), used.size() * 4) == 0, "allele_probes");
    uint64_t n_selected = 0;
    for (uint64_t c = 0; c < n_cols; c++) n_selected += selected(c);
    std::vector<uint32_t> carried(n_cols, 0), called(n_cols, 0);
    for (uint32_t v = 0; v < n_variants; v++) {
        uint32_t n[4] = {0, 0, 0, 0};
        for (uint64_t c = 0; c < n_cols; c++) {
            const bool r = bit(&want[0][v * rb], c), a = bit(&want[1][v * rb], c);
            CHECK(selected(c) || (!r && !a), "an unselected column holds a bit");
            if (!selected(c)) continue;
            n[r ? (a ? 1 : 0) : (a ? 2 : 3)]++;
            carried[c] += a;
            called[c] += r || a;
        }
        CHECK(memcmp(&vc[v * 4], n, sizeof n) == 0 && n[0] + n[1] + n[2] + n[3] == n_selected, "the counts of variant %u", v);
    }
    for (uint64_t c = 0; c < n_cols; c++) CHECK(sc[c * 2] == carried[c] && sc[c * 2 + 1] == called[c], "the counts of column %llu", (unsigned long long)c);
    // without planes: the same counts, the plane buffers untouched
    std::vector<uint32_t> vc2(n_variants * 4), sc2(n_cols * 2), ap2(n_variants * 2);
    CHECK(bigsi_cpu_genotype(ix, blob.data(), off.data(), n_seqs, k, threshold, allele_of.data(), n_variants, cols, nullptr, nullptr, 0, vc2.data(), sc2.data(), n_cols, ap2.data()) == 0,
          "%s", bigsi_cpu_last_error());
    CHECK(memcmp(vc2.data(), vc.data(), vc2.size() * 4) == 0 && memcmp(sc2.data(), sc.data(), sc2.size() * 4) == 0 && memcmp(ap2.data(), ap.data(), ap2.size() * 4) == 0, "NULL planes");
    CHECK(bigsi_cpu_close(ix) == 0, "%s", bigsi_cpu_last_error());
}

int main()
{
    planner();
    for (uint64_t n_cols : {1ull, 63ull, 64ull, 65ull, 127ull, 129ull, 200ull})
        for (double t : {1.0, 0.5, 0.0, -1.0})
            for (uint64_t n_seqs : {1ull, 2ull, 9ull})
                for (uint32_t n_variants : {1u, 3u, 65u})
                    for (bool masked : {false, true}) twin(97, n_cols, 2, 5, n_seqs, t, n_variants, masked);
    printf("genotype planner and twin: ok\n");
    return 0;
}
