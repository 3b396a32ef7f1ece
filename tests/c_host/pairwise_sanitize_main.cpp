// A stand-alone program (its own main) that drives the host side of the pairwise popcounts -- plan_pairwise and pairwise_tables
// (bigsi_amd/csrc/bigsi_launch.hpp), the replay of the three kernels from them (pairwise_host.cpp) -- and the CPU twin's
// bigsi_cpu_pairwise_popcounts (bigsi_amd/cpu/bigsi_cpu.cpp) over odd shapes, checks both against a naive count of shared bits, and
// is meant to be built with -fsanitize=address,undefined and run on the CPU: tests/test_pairwise_host.py compiles it together with
// bigsi_cpu.cpp and runs it.  Nothing sanitized is loaded into Python.
// Test infrastructure only: nothing in the product loads this file.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "pairwise_host.cpp"
#include "bigsi_cpu_pairwise.h"

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

static bool get_bit(const uint8_t *row, uint64_t c) { return row[c >> 3] & (0x80u >> (c & 7)); }

static void one_shape(uint64_t m, uint64_t n, uint64_t na, uint64_t nb, bool symmetric)
{
    bigsi_cpu_index *ix = nullptr;
    CHECK(bigsi_cpu_open(m, n, n, 3, 0, &ix) == 0, "%s", bigsi_cpu_last_error());
    bigsi_hip_info info;
    CHECK(bigsi_cpu_get_info(ix, &info) == 0, "%s", bigsi_cpu_last_error());
    const uint64_t stride = info.row_stride_bytes;
    std::vector<uint8_t> rows(m * stride);          // (junk behind num_cols too: no selected column reads it)
    for (auto &b : rows) b = (uint8_t)(rnd() & rnd());
    std::vector<uint64_t> ids(m);
    for (uint64_t r = 0; r < m; r++) ids[r] = r;
    CHECK(bigsi_cpu_set_rows(ix, ids.data(), m, rows.data(), stride) == 0, "%s", bigsi_cpu_last_error());
    std::vector<uint32_t> a(na), b(nb);
    for (auto &c : a) c = (uint32_t)(rnd() % n);          // (repeats and any order)
    for (auto &c : b) c = (uint32_t)(rnd() % n);
    a[0] = (uint32_t)(n - 1);
    if (symmetric) b = a;
    const uint64_t nbb = b.size();
    std::vector<uint64_t> want(na * nbb, 0), twin(na * nbb, 0xABABABABABABABABull), again(na * nbb, 0xABABABABABABABABull);
    for (uint64_t r = 0; r < m; r++)
        for (uint64_t i = 0; i < na; i++)
            for (uint64_t j = 0; j < nbb; j++) want[i * nbb + j] += get_bit(rows.data() + r * stride, a[i]) && get_bit(rows.data() + r * stride, b[j]);
    CHECK(bigsi_cpu_pairwise_popcounts(ix, a.data(), na, symmetric ? nullptr : b.data(), symmetric ? 0 : nbb, twin.data(), twin.size()) == 0, "%s",
          bigsi_cpu_last_error());
    CHECK(twin == want, "the twin on %llu x %llu, %llu x %llu", (unsigned long long)m, (unsigned long long)n, (unsigned long long)na, (unsigned long long)nbb);
    const int rc = pairwise_host_replay(rows.data(), m, stride, a.data(), na, symmetric ? nullptr : b.data(), nbb, again.data());
    CHECK(rc == 0, "the replay's invariant %d on %llu x %llu", rc, (unsigned long long)m, (unsigned long long)n);
    CHECK(again == want, "the replay on %llu x %llu, %llu x %llu", (unsigned long long)m, (unsigned long long)n, (unsigned long long)na, (unsigned long long)nbb);
    // refusals leave out as it is
    std::vector<uint64_t> keep(twin);
    a[na / 2] = (uint32_t)n;
    CHECK(bigsi_cpu_pairwise_popcounts(ix, a.data(), na, nullptr, 0, twin.data(), 0) == BIGSI_ERR_RANGE, "a column out of range (named before the capacity)");
    CHECK(bigsi_cpu_pairwise_popcounts(ix, b.data(), nbb, nullptr, 0, twin.data(), nbb * nbb - 1) == BIGSI_ERR_CAPACITY, "a short out");
    CHECK(bigsi_cpu_pairwise_popcounts(ix, b.data(), 0, nullptr, 0, twin.data(), twin.size()) == BIGSI_ERR_INVALID, "an empty list");
    CHECK(twin == keep, "a refused call wrote to out");
    CHECK(bigsi_cpu_close(ix) == 0, "%s", bigsi_cpu_last_error());
}

int main()
{
    const uint64_t T = bigsi::kPairTile;
    for (uint64_t m : {(uint64_t)1, (uint64_t)63, (uint64_t)64, (uint64_t)65, (uint64_t)257, (uint64_t)2047, (uint64_t)2048, (uint64_t)2049, (uint64_t)4100})
        for (uint64_t n : {(uint64_t)1, (uint64_t)65, (uint64_t)129, (uint64_t)1025})
            for (uint64_t s : {(uint64_t)1, (uint64_t)2, T - 1, T + 1}) {
                if (m > 300 && s > 2 && n != 129) continue;          // (the naive count is m x s x s)
                one_shape(m, n, s, s, true);
                one_shape(m, n, s, 3, false);
                one_shape(m, n, 1, s, false);
            }
    one_shape(130, 300, 2 * T + 1, 2 * T + 1, true);
    printf("pairwise planner, replay and twin: ok\n");
    return 0;
}
