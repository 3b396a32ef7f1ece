// A stand-alone program (its own main) that drives the exact k-mer counter of libbigsi_cpu.so, bigsi_cpu_kmer_counter_*
// (bigsi_amd/cpu/bigsi_cpu.cpp), over odd shapes, checks it against a count taken here base by base, and is meant to be built with
// -fsanitize=address,undefined and run on the CPU: tests/test_kmercount_host.py compiles it together with bigsi_cpu.cpp and runs it.
// Nothing sanitized is loaded into Python.
// Test infrastructure only: nothing in the product loads this file.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include <algorithm>
#include "bigsi_cpu_kmercount.h"

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

// the counter against a count taken here, the plainest way: strings in a std::map
static void twin(uint32_t k, const std::vector<std::string> &seqs, uint64_t m, uint32_t h)
{
    std::string blob;
    std::vector<uint64_t> off(1, 0);
    for (const std::string &s : seqs) { blob += s; off.push_back(blob.size()); }
    std::map<std::string, uint32_t> want;
    uint64_t counted = 0, skipped = 0;
    for (const std::string &s : seqs)
        for (size_t p = 0; p + k <= s.size(); p++) {
            std::string f = s.substr(p, k), r(k, 'N');
            bool ok = true;
            for (uint32_t j = 0; j < k; j++) {
                char c = f[j];
                if (c >= 'a' && c <= 'z') c = (char)(c - 32);
                f[j] = c;
                ok = ok && (c == 'A' || c == 'C' || c == 'G' || c == 'T');
                r[k - 1 - j] = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
            }
            if (!ok) { skipped++; continue; }
            counted++;
            want[std::min(f, r)]++;
        }
    bigsi_cpu_kmer_counter *c = nullptr;
    CHECK(bigsi_cpu_kmer_counter_create(0, k, 0, &c) == BIGSI_OK, "create: %s", bigsi_cpu_last_error());
    // in two calls, the second one through offsets that do not start at 0
    const uint64_t half = seqs.size() / 2;
    CHECK(bigsi_cpu_kmer_counter_add(c, blob.data(), off.data(), half) == BIGSI_OK, "add: %s", bigsi_cpu_last_error());
    CHECK(bigsi_cpu_kmer_counter_add(c, blob.data(), off.data() + half, seqs.size() - half) == BIGSI_OK, "add: %s", bigsi_cpu_last_error());
    uint64_t info[4];
    CHECK(bigsi_cpu_kmer_counter_info(c, info) == BIGSI_OK, "info");
    CHECK(info[0] == counted && info[1] == skipped && info[2] == want.size(), "info %llu %llu %llu", (unsigned long long)info[0], (unsigned long long)info[1], (unsigned long long)info[2]);
    uint64_t n = 0;
    CHECK(bigsi_cpu_kmer_counter_fetch(c, nullptr, nullptr, 0, &n) == (want.empty() ? BIGSI_OK : BIGSI_ERR_CAPACITY) && n == want.size(), "the sizing call");
    std::vector<uint64_t> keys(n + 1, 0xABABABABABABABABull);
    std::vector<uint32_t> counts(n + 1, 0xABABABABu);
    CHECK(bigsi_cpu_kmer_counter_fetch(c, keys.data(), counts.data(), n, &n) == BIGSI_OK, "fetch: %s", bigsi_cpu_last_error());
    CHECK(keys[n] == 0xABABABABABABABABull && counts[n] == 0xABABABABu, "fetch wrote beyond its entries");
    uint64_t spectrum[256], want_spectrum[256] = {0};
    size_t i = 0;
    std::string kept;
    for (const auto &kv : want) {          // (the map's order is the keys' order: the strings sort as the packed keys do)
        uint64_t key = 0;
        for (char ch : kv.first) key = (key << 2) | (uint64_t)(ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : 3);
        CHECK(keys[i] == key && counts[i] == kv.second, "entry %zu", i);
        want_spectrum[std::min<uint32_t>(kv.second, 255)]++;
        if (kv.second >= 2) kept += kv.first;
        i++;
    }
    CHECK(bigsi_cpu_kmer_counter_spectrum(c, spectrum) == BIGSI_OK && memcmp(spectrum, want_spectrum, sizeof spectrum) == 0, "spectrum");
    const uint64_t nb = (m + 7) / 8;
    std::vector<uint8_t> got(nb + 1, 0xCD), ref(nb, 0);
    CHECK(bigsi_cpu_kmer_counter_bloom(c, m, h, 2, got.data()) == BIGSI_OK, "bloom: %s", bigsi_cpu_last_error());
    CHECK(bigsi_cpu_bloom(0, kept.data(), kept.size() / k, k, m, h, 0, ref.data()) == BIGSI_OK, "bigsi_cpu_bloom");
    CHECK(got[nb] == 0xCD && memcmp(got.data(), ref.data(), nb) == 0, "the filter differs from bigsi_cpu_bloom of the kept k-mers");
    CHECK(bigsi_cpu_kmer_counter_bloom(c, m, h, 0, got.data()) == BIGSI_ERR_INVALID, "min_count 0");
    CHECK(bigsi_cpu_kmer_counter_reset(c) == BIGSI_OK && bigsi_cpu_kmer_counter_info(c, info) == BIGSI_OK && info[0] + info[1] + info[2] == 0, "reset");
    CHECK(bigsi_cpu_kmer_counter_destroy(c) == BIGSI_OK, "destroy");
}

int main()
{
    const char alphabet[] = "ACGTacgtN";
    for (uint32_t k : {1u, 2u, 16u, 31u, 32u}) {
        std::vector<std::string> seqs = {"", std::string(k - 1, 'A'), std::string(k, 'T'), std::string(k + 7, 'A'), std::string(40, 'N')};
        for (int i = 0; i < 40; i++) {
            std::string s(rnd() % 90, 'A');
            for (char &ch : s) ch = alphabet[rnd() % (i % 4 == 0 ? 9 : 4)];
            seqs.push_back(s);
            if (i % 5 == 0) seqs.push_back(s);          // repeats: counts above 1
        }
        seqs.push_back(std::string("AC\0GT>ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGT", 46));
        twin(k, seqs, k % 2 ? 1000 : 33, 1 + k % 3);
    }
    bigsi_cpu_kmer_counter *c = nullptr;
    CHECK(bigsi_cpu_kmer_counter_create(0, 33, 0, &c) == BIGSI_ERR_INVALID && !c, "k = 33");
    CHECK(bigsi_cpu_kmer_counter_create(0, 0, 0, &c) == BIGSI_ERR_INVALID && !c, "k = 0");
    printf("kmercount: ok\n");
    return 0;
}
