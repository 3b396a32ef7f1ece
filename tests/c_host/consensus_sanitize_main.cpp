// A stand-alone program (its own main) that drives the host planner of the consensus collapse (plan_consensus_columns,
// bigsi_amd/csrc/bigsi_launch.hpp) and the CPU twin's bigsi_cpu_consensus_columns_into (bigsi_amd/cpu/bigsi_cpu.cpp) over odd shapes,
// checks both against a naive count of members, and is meant to be built with -fsanitize=address,undefined and run on the CPU:
// tests/test_consensus_columns_host.py compiles it together with bigsi_cpu.cpp and runs it.  Nothing sanitized is loaded into Python.
// Test infrastructure only: nothing in the product loads this file.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../bigsi_amd/csrc/bigsi_launch.hpp"
#include "bigsi_cpu_consensus.h"

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

// the kernel's arithmetic on one row, from the plan's tables: the source as little-endian 32-bit words, the image as 32-bit words of
// packed fields (adds that wrap like the device's), window by window; the read-out lane by lane
static void replay(const bigsi::ConsensusPlan &p, const uint8_t *src_row, std::vector<uint8_t> &dst_row)
{
    const uint32_t fb = p.field_bits, per = 32 / fb, mask = fb == 32 ? 0xFFFFFFFFu : (1u << fb) - 1u;
    dst_row.assign(round_up(p.dst_words, 2) * 8, 0);
    std::vector<uint32_t> img(p.image_words * 2, 0);
    for (uint64_t j = 0; j < p.windows; j++) {
        uint64_t win0, win_n;
        bigsi::consensus_window(p, j, &win0, &win_n);
        const uint32_t lo = (uint32_t)(win0 * 64), span = (uint32_t)(win_n * 64);
        for (uint64_t d = 0; d < p.table_words * 2; d++) {
            uint32_t x, l;
            memcpy(&x, src_row + d * 4, 4);
            memcpy(&l, reinterpret_cast<const uint8_t *>(p.live.data()) + d * 4, 4);
            for (x &= l; x; x &= x - 1) {
                const uint32_t a = p.dst_col[d * 32 + (uint32_t)__builtin_ctz(x)] - lo;
                if (a < span) img[a / per] += 1u << ((a % per) * fb);
            }
        }
        const uint64_t pair_n = round_up(win_n, 2);
        CHECK(pair_n * 2 * fb <= img.size(), "the read-out of window %llu leaves the image", (unsigned long long)j);
        for (uint64_t w = 0; w < pair_n; w++) {
            uint64_t word = 0;
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint32_t c = (uint32_t)w * 64 + (lane ^ 7u);
                CHECK((win0 + w) * 64 + lane < p.need.size(), "the read-out of window %llu leaves the need table", (unsigned long long)j);
                if (((img[c / per] >> ((c % per) * fb)) & mask) >= p.need[(win0 + w) * 64 + lane]) word |= 1ull << lane;
            }
            memcpy(dst_row.data() + (win0 + w) * 8, &word, 8);          // (a little-endian host, as the device)
        }
        for (uint64_t i = 0; i < pair_n * 2 * fb; i++) img[i] = 0;
    }
    for (uint32_t v : img) CHECK(v == 0, "the image is clear after the last window");
}

// sizes_mode 0: random groups; 1: consecutive groups of exactly 255 members (8-bit fields at their maximum beside each other)
static void one_shape(uint64_t m, uint64_t n, uint64_t groups, int drop_percent, uint64_t window_words, int sizes_mode, int need_mode)
{
    std::vector<uint32_t> group_of(n ? n : 1), size(groups, 0), need(groups);
    for (uint64_t c = 0; c < n; c++) {
        if (sizes_mode == 1) group_of[c] = c / 255 < groups ? (uint32_t)(c / 255) : bigsi::kCollapseDropped;
        else group_of[c] = (int)(rnd() % 100) < drop_percent ? bigsi::kCollapseDropped : (uint32_t)(rnd() % groups);
        if (group_of[c] != bigsi::kCollapseDropped) size[group_of[c]]++;
    }
    for (uint64_t g = 0; g < groups; g++)
        need[g] = need_mode == 0 ? 1u : need_mode == 1 ? (size[g] ? size[g] : 1u) : 1u + (uint32_t)(rnd() % (size[g] + 1));
    bigsi_cpu_index *src = nullptr, *dst = nullptr;
    CHECK(bigsi_cpu_open(m, n, n, 3, 0, &src) == 0 && bigsi_cpu_open(m, 0, 1, 3, 0, &dst) == 0, "%s", bigsi_cpu_last_error());
    bigsi_hip_info info;
    CHECK(bigsi_cpu_get_info(src, &info) == 0, "%s", bigsi_cpu_last_error());
    const uint64_t src_stride = info.row_stride_bytes;
    // rows at the full stride: the junk behind num_cols is part of what must not count; row 0 is all ones (the fields at their maximum)
    std::vector<uint8_t> rows(m * src_stride);
    for (auto &b : rows) b = (uint8_t)rnd();
    memset(rows.data(), 0xFF, src_stride);
    std::vector<uint64_t> ids(m);
    for (uint64_t r = 0; r < m; r++) ids[r] = r;
    CHECK(bigsi_cpu_set_rows(src, ids.data(), m, rows.data(), src_stride) == 0, "%s", bigsi_cpu_last_error());
    // refusals leave the destination as it is
    if (groups > 1) {
        std::vector<uint32_t> zero(need);
        zero[groups - 1] = 0;
        CHECK(bigsi_cpu_consensus_columns_into(dst, src, group_of.data(), groups, zero.data()) == BIGSI_ERR_INVALID, "a zero in min_members");
    }
    CHECK(bigsi_cpu_consensus_columns_into(dst, src, group_of.data(), groups, nullptr) == BIGSI_ERR_INVALID, "min_members NULL");
    CHECK(bigsi_cpu_get_info(dst, &info) == 0 && info.num_cols == 0, "a refused call left columns behind");
    CHECK(bigsi_cpu_consensus_columns_into(dst, src, group_of.data(), groups, need.data()) == 0, "%s", bigsi_cpu_last_error());
    CHECK(bigsi_cpu_get_info(dst, &info) == 0 && info.num_cols == groups, "num_cols %llu", (unsigned long long)info.num_cols);
    const uint64_t dst_stride = info.row_stride_bytes;
    std::vector<uint8_t> got(m * dst_stride, 0xAB), want(dst_stride), again;
    std::vector<uint32_t> count(groups);
    CHECK(bigsi_cpu_get_rows(dst, ids.data(), m, got.data(), dst_stride) == 0, "%s", bigsi_cpu_last_error());
    const bigsi::ConsensusPlan p = bigsi::plan_consensus_columns(n, group_of.data(), groups, need.data(), m, window_words);
    const uint64_t field_max = p.field_bits == 32 ? 0xFFFFFFFFull : (1ull << p.field_bits) - 1;
    CHECK(p.window_words % 2 == 0 && p.image_words % (2 * p.field_bits) == 0 && p.lds_bytes <= bigsi::kCollapseLdsBytes && p.largest <= field_max,
          "the plan's LDS and field invariants");
    CHECK(p.table_words * 8 <= src_stride, "table_words %llu passes the source stride", (unsigned long long)p.table_words);
    for (uint64_t g = 0; g < groups; g++) CHECK(p.sizes[g] == size[g], "the size of group %llu", (unsigned long long)g);
    for (uint64_t r = 0; r < m; r++) {
        const uint8_t *x = rows.data() + r * src_stride;
        memset(want.data(), 0, dst_stride);
        std::fill(count.begin(), count.end(), 0u);
        for (uint64_t c = 0; c < n; c++)
            if (group_of[c] != bigsi::kCollapseDropped && get_bit(x, c)) count[group_of[c]]++;
        for (uint64_t g = 0; g < groups; g++)
            if (count[g] >= need[g]) want[g >> 3] |= (uint8_t)(0x80u >> (g & 7));
        CHECK(memcmp(want.data(), got.data() + r * dst_stride, dst_stride) == 0, "the twin's row %llu of %llu x %llu -> %llu", (unsigned long long)r,
              (unsigned long long)m, (unsigned long long)n, (unsigned long long)groups);
        replay(p, x, again);
        CHECK(again.size() <= dst_stride && memcmp(want.data(), again.data(), again.size()) == 0, "the replayed row %llu of %llu x %llu -> %llu (window %llu, %u-bit fields)",
              (unsigned long long)r, (unsigned long long)m, (unsigned long long)n, (unsigned long long)groups, (unsigned long long)p.window_words, p.field_bits);
    }
    CHECK(bigsi_cpu_consensus_columns_into(dst, src, group_of.data(), groups, need.data()) == BIGSI_ERR_STATE, "a destination that holds columns");
    CHECK(bigsi_cpu_consensus_columns_into(src, src, group_of.data(), groups, need.data()) == BIGSI_ERR_INVALID, "dst == src");
    CHECK(bigsi_cpu_close(src) == 0 && bigsi_cpu_close(dst) == 0, "%s", bigsi_cpu_last_error());
}

int main()
{
    const uint64_t widths[] = {0, 1, 8, 63, 64, 65, 127, 128, 129, 1023, 1025, 8191, 8193};
    int turn = 0;
    for (uint64_t n : widths)
        for (uint64_t groups : {(uint64_t)1, (uint64_t)3, (uint64_t)64, (uint64_t)65, (uint64_t)129, n + 1, 2 * n + 7})
            for (int drop : {0, 30, 100})
                for (uint64_t window : {(uint64_t)0, (uint64_t)2, (uint64_t)6}) one_shape(n > 1000 ? 3 : 5, n, groups, drop, window, 0, turn++ % 3);
    // 8-bit fields at their maximum beside each other, 16-bit fields (one group of 8193), several windows of the planner as committed
    for (uint64_t window : {(uint64_t)0, (uint64_t)2})
        for (int need_mode : {0, 1, 2}) one_shape(3, 255 * 9 + 17, 9, 0, window, 1, need_mode);
    one_shape(2, 8193, 1, 0, 0, 0, 1);
    one_shape(2, 3000, 2 * (bigsi::kCollapseWindowWords / 8) * 64 + 70, 10, 0, 0, 2);
    printf("consensus planner and twin: ok\n");
    return 0;
}
