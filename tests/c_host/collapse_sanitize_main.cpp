// A stand-alone program (its own main) that drives the host planner of the column collapse (plan_collapse_columns,
// bigsi_amd/csrc/bigsi_launch.hpp) and the CPU twin's bigsi_cpu_collapse_columns_into (bigsi_amd/cpu/bigsi_cpu.cpp) over odd shapes,
// checks both against a naive OR of columns, and is meant to be built with -fsanitize=address,undefined and run on the CPU:
// tests/test_collapse_columns_host.py compiles it together with bigsi_cpu.cpp and runs it.  Nothing sanitized is loaded into Python.
// Test infrastructure only: nothing in the product loads this file.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../bigsi_amd/csrc/bigsi_launch.hpp"
#include "bigsi_cpu_collapse.h"

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

// the kernel's arithmetic on one row, from the plan's tables: source and image as little-endian 32-bit words, window by window
static void replay(const bigsi::CollapsePlan &p, const uint8_t *src_row, std::vector<uint8_t> &dst_row)
{
    dst_row.assign(round_up(p.dst_words, 2) * 8, 0);
    std::vector<uint32_t> img(p.image_words * 2, 0);
    for (uint64_t j = 0; j < p.windows; j++) {
        uint64_t win0, win_n;
        bigsi::collapse_window(p, j, &win0, &win_n);
        const uint32_t lo = (uint32_t)(win0 * 64), span = (uint32_t)(win_n * 64);
        for (uint64_t d = 0; d < p.table_words * 2; d++) {
            uint32_t x, l;
            memcpy(&x, src_row + d * 4, 4);
            memcpy(&l, reinterpret_cast<const uint8_t *>(p.live.data()) + d * 4, 4);
            for (x &= l; x; x &= x - 1) {
                const uint32_t a = p.dst_bit[d * 32 + (uint32_t)__builtin_ctz(x)] - lo;
                if (a < span) img[a >> 5] |= 1u << (a & 31u);
            }
        }
        for (uint64_t i = 0; i < win_n; i += 2) {
            CHECK(2 * i + 4 <= img.size(), "the read-out of window %llu leaves the image", (unsigned long long)j);
            memcpy(dst_row.data() + (win0 + i) * 8, img.data() + 2 * i, 16);
            memset(img.data() + 2 * i, 0, 16);
        }
    }
}

static void one_shape(uint64_t m, uint64_t n, uint64_t groups, int drop_percent, uint64_t window_words)
{
    std::vector<uint32_t> group_of(n ? n : 1);
    for (uint64_t c = 0; c < n; c++) group_of[c] = (int)(rnd() % 100) < drop_percent ? bigsi::kCollapseDropped : (uint32_t)(rnd() % groups);
    bigsi_cpu_index *src = nullptr, *dst = nullptr;
    CHECK(bigsi_cpu_open(m, n, n, 3, 0, &src) == 0 && bigsi_cpu_open(m, 0, 1, 3, 0, &dst) == 0, "%s", bigsi_cpu_last_error());
    bigsi_hip_info info;
    CHECK(bigsi_cpu_get_info(src, &info) == 0, "%s", bigsi_cpu_last_error());
    const uint64_t src_stride = info.row_stride_bytes;
    // rows at the full stride: the junk behind num_cols is part of what must not survive
    std::vector<uint8_t> rows(m * src_stride);
    for (auto &b : rows) b = (uint8_t)rnd();
    std::vector<uint64_t> ids(m);
    for (uint64_t r = 0; r < m; r++) ids[r] = r;
    CHECK(bigsi_cpu_set_rows(src, ids.data(), m, rows.data(), src_stride) == 0, "%s", bigsi_cpu_last_error());
    CHECK(bigsi_cpu_collapse_columns_into(dst, src, group_of.data(), groups) == 0, "%s", bigsi_cpu_last_error());
    CHECK(bigsi_cpu_get_info(dst, &info) == 0 && info.num_cols == groups, "num_cols %llu", (unsigned long long)info.num_cols);
    const uint64_t dst_stride = info.row_stride_bytes;
    std::vector<uint8_t> got(m * dst_stride, 0xAB), want(dst_stride), again;
    CHECK(bigsi_cpu_get_rows(dst, ids.data(), m, got.data(), dst_stride) == 0, "%s", bigsi_cpu_last_error());
    const bigsi::CollapsePlan p = window_words ? bigsi::plan_collapse_columns(n, group_of.data(), groups, m, window_words)
                                               : bigsi::plan_collapse_columns(n, group_of.data(), groups, m);
    CHECK(p.image_words % 2 == 0 && p.image_words <= p.window_words && p.lds_bytes <= bigsi::kCollapseLdsBytes, "the plan's LDS invariants");
    CHECK(p.table_words * 8 <= src_stride, "table_words %llu passes the source stride", (unsigned long long)p.table_words);
    for (uint64_t r = 0; r < m; r++) {
        const uint8_t *x = rows.data() + r * src_stride;
        memset(want.data(), 0, dst_stride);
        for (uint64_t c = 0; c < n; c++)
            if (group_of[c] != bigsi::kCollapseDropped && get_bit(x, c)) want[group_of[c] >> 3] |= (uint8_t)(0x80u >> (group_of[c] & 7));
        CHECK(memcmp(want.data(), got.data() + r * dst_stride, dst_stride) == 0, "the twin's row %llu of %llu x %llu -> %llu", (unsigned long long)r,
              (unsigned long long)m, (unsigned long long)n, (unsigned long long)groups);
        replay(p, x, again);
        CHECK(again.size() <= dst_stride && memcmp(want.data(), again.data(), again.size()) == 0, "the replayed row %llu of %llu x %llu -> %llu (window %llu)",
              (unsigned long long)r, (unsigned long long)m, (unsigned long long)n, (unsigned long long)groups, (unsigned long long)p.window_words);
    }
    // refusals leave the destination as it is
    CHECK(bigsi_cpu_collapse_columns_into(dst, src, group_of.data(), groups) == BIGSI_ERR_STATE, "a destination that holds columns");
    CHECK(bigsi_cpu_collapse_columns_into(src, src, group_of.data(), groups) == BIGSI_ERR_INVALID, "dst == src");
    CHECK(bigsi_cpu_close(src) == 0 && bigsi_cpu_close(dst) == 0, "%s", bigsi_cpu_last_error());
}

int main()
{
    const uint64_t widths[] = {0, 1, 8, 63, 64, 65, 127, 128, 129, 1023, 1025, 8191, 8193};
    for (uint64_t n : widths)
        for (uint64_t groups : {(uint64_t)1, (uint64_t)3, (uint64_t)64, (uint64_t)65, (uint64_t)129, n + 1, 2 * n + 7})
            for (int drop : {0, 30, 100})
                for (uint64_t window : {(uint64_t)0, (uint64_t)2, (uint64_t)6}) one_shape(n > 1000 ? 3 : 7, n, groups, drop, window);
    // several windows of the planner as committed
    one_shape(2, 3000, 2 * bigsi::kCollapseWindowWords * 64 + 70, 10, 0);
    printf("collapse planner and twin: ok\n");
    return 0;
}
