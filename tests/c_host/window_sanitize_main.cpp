// A stand-alone program (its own main) that drives the host planner of the windowed search (plan_window_search,
// bigsi_amd/csrc/bigsi_launch.hpp) and the CPU twin's bigsi_cpu_window_search (bigsi_amd/cpu/bigsi_cpu.cpp) over edge shapes, checks
// the planner's invariants and the twin against a brute-force count of its own, and is meant to be built with
// -fsanitize=address,undefined and run on the CPU: tests/test_window_host.py compiles it together with bigsi_cpu.cpp and runs it.
// Nothing sanitized is loaded into Python.
// Test infrastructure only: nothing in the product loads this file.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../bigsi_amd/csrc/bigsi_launch.hpp"
#include "bigsi_cpu_window.h"

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

static void plan_shape(const std::vector<uint32_t> &n, uint32_t window, uint64_t wv, uint32_t h, uint64_t forced, uint64_t cap)
{
    const bigsi::WindowPlan p = bigsi::plan_window_search(n.data(), (uint32_t)n.size(), window, wv, h, forced, cap);
    CHECK(p.seg_off.size() == n.size() + 1 && p.seg_off.back() == p.segs.size() && p.n_segs == p.segs.size(), "segment offsets");
    uint32_t max_we = 0;
    for (size_t q = 0; q < n.size(); q++) {
        const uint32_t we = std::min(n[q], window);
        max_we = std::max(max_we, we);
        uint64_t next = 0;
        for (uint64_t s = p.seg_off[q]; s < p.seg_off[q + 1]; s++) {
            const bigsi::WindowSeg &g = p.segs[s];
            CHECK(g.q == q && g.we == we && g.a == next && g.a < g.b && g.b - g.a <= p.seg_starts, "segment %llu of sequence %zu", (unsigned long long)s, q);
            next = g.b;
        }
        CHECK(next == (we ? (uint64_t)n[q] - we + 1 : 0), "the segments of sequence %zu end at %llu", q, (unsigned long long)next);
    }
    CHECK(p.max_we == max_we && p.planes >= bigsi::window_bit_width(max_we) && p.planes <= 16 && p.planes % 4 == 0 && p.planes >= 4, "planes %u for %u", p.planes, max_we);
    CHECK(p.wvp % 2 == 0 && p.wvp >= wv && p.wvp < wv + 2, "wvp %llu", (unsigned long long)p.wvp);
    CHECK(p.partial_bytes == p.n_segs * p.planes * p.wvp * 8, "partial bytes");
    CHECK(p.tiles * 128ull >= wv && p.waves == p.n_segs * p.tiles && p.grid * 4 >= p.waves && (p.grid == 0 || (p.grid - 1) * 4 < p.waves), "grid");
    CHECK(p.grid_too_large == (p.grid > 0x7FFFFFFFull), "grid refusal");
    CHECK(p.partial_too_large == (p.partial_bytes > (cap ? cap : bigsi::kWindowPartialBytes)), "partial refusal");
}

static void planners()
{
    for (uint32_t window : {1u, 2u, 3u, 15u, 16u, 255u, 256u, 4095u, 4096u, 65535u})
        for (uint64_t wv : {1ull, 2ull, 3ull, 128ull, 129ull, 1563ull})
            for (uint32_t h : {1u, 3u, 9u})
                for (uint64_t forced : {0ull, 1ull, 64ull}) {
                    std::vector<uint32_t> n = {0, 1, window, window > 1 ? window - 1 : 1, window + 1, 3000, (uint32_t)(rnd() % 5000), 0};
                    plan_shape(n, window, wv, h, forced, 0);
                    plan_shape(n, window, wv, h, forced, 4096);
                }
    plan_shape({}, 5, 10, 3, 0, 0);
    plan_shape({0, 0}, 5, 10, 3, 0, 0);
    plan_shape({100000}, 1000, 1563, 4, 0, 0);
}

static void twin(uint64_t m, uint64_t n_cols, uint32_t h, uint32_t k, uint32_t window, double threshold)
{
    bigsi_cpu_index *ix = nullptr;
    CHECK(bigsi_cpu_open(m, n_cols, n_cols, h, 0, &ix) == 0, "%s", bigsi_cpu_last_error());
    bigsi_hip_info info;
    CHECK(bigsi_cpu_get_info(ix, &info) == 0, "%s", bigsi_cpu_last_error());
    const uint64_t stride = info.row_stride_bytes;
    std::vector<uint8_t> rows(m * stride);
    for (auto &b : rows) b = (uint8_t)(rnd() | rnd());          // dense rows, junk behind num_cols included
    std::vector<uint64_t> ids(m);
    for (uint64_t r = 0; r < m; r++) ids[r] = r;
    CHECK(bigsi_cpu_set_rows(ix, ids.data(), m, rows.data(), stride) == 0, "%s", bigsi_cpu_last_error());
    const uint64_t lens[6] = {k - 1ull, k, k + window - 2ull + (window == 1), k + window - 1ull, k + window + 5ull, 0ull};
    std::string blob;
    std::vector<uint64_t> off(7, 0);
    for (int i = 0; i < 6; i++) {
        for (uint64_t j = 0; j < lens[i]; j++) blob.push_back("AC"[rnd() & 1]);          // two letters: repeated k-mers
        off[i + 1] = blob.size();
    }
    const uint64_t cap = 6 * n_cols;
    std::vector<uint32_t> used(7, 0xABABABABu), need(7, 0xABABABABu), col(cap + 1, 0xABABABABu);
    std::vector<uint64_t> hoff(8, 0xABABABABABABABABull);
    std::vector<bigsi_hip_window_hit> rec(cap + 1);
    memset(rec.data(), 0xAB, rec.size() * sizeof rec[0]);
    CHECK(bigsi_cpu_window_search(ix, blob.data(), off.data(), 6, k, 0, threshold, used.data(), need.data(), hoff.data(), col.data(), rec.data(), cap) == BIGSI_ERR_INVALID, "window 0");
    CHECK(bigsi_cpu_window_search(ix, blob.data(), off.data(), 6, k, 65536, threshold, used.data(), need.data(), hoff.data(), col.data(), rec.data(), cap) == BIGSI_ERR_INVALID, "window 65536");
    CHECK(bigsi_cpu_window_search(ix, blob.data(), off.data(), 6, k, window, 0.0, used.data(), need.data(), hoff.data(), col.data(), rec.data(), cap) == BIGSI_ERR_INVALID, "threshold 0");
    CHECK(bigsi_cpu_window_search(ix, blob.data(), off.data(), 6, k, window, 1.5, used.data(), need.data(), hoff.data(), col.data(), rec.data(), cap) == BIGSI_ERR_INVALID, "threshold 1.5");
    CHECK(bigsi_cpu_window_search(ix, blob.data(), off.data(), 6, k, window, threshold, nullptr, need.data(), hoff.data(), col.data(), rec.data(), cap) == BIGSI_ERR_INVALID, "NULL");
    CHECK(used[0] == 0xABABABABu && hoff[0] == 0xABABABABABABABABull, "a refused call wrote its outputs");
    CHECK(bigsi_cpu_window_search(ix, blob.data(), off.data(), 6, k, window, threshold, used.data(), need.data(), hoff.data(), col.data(), rec.data(), cap) == 0, "%s", bigsi_cpu_last_error());
    CHECK(used[6] == 0xABABABABu && need[6] == 0xABABABABu && hoff[7] == 0xABABABABABABABABull && col[cap] == 0xABABABABu, "wrote behind an output");
    const uint64_t total = hoff[6];
    // brute force from the presence strings of the twin itself
    uint64_t at = 0;
    for (int i = 0; i < 6; i++) {
        const uint64_t n = lens[i] >= k ? lens[i] - k + 1 : 0;
        const uint32_t we = (uint32_t)std::min<uint64_t>(n, window), thr = (uint32_t)ceil((double)we * threshold);
        CHECK(used[i] == we && need[i] == thr && hoff[i] == at, "sequence %d: window %u need %u", i, used[i], need[i]);
        if (!n) continue;
        std::vector<uint32_t> all(n_cols);
        for (uint64_t c = 0; c < n_cols; c++) all[c] = (uint32_t)c;
        std::vector<uint8_t> pres(n_cols * n);
        CHECK(bigsi_cpu_presence(ix, blob.data() + off[i], lens[i], k, all.data(), (uint32_t)n_cols, pres.data()) == 0, "%s", bigsi_cpu_last_error());
        for (uint64_t c = 0; c < n_cols; c++) {
            bigsi_hip_window_hit w{0, 0, 0, 0, 0, 0};
            for (uint64_t s = 0; s + we <= n; s++) {
                uint32_t f = 0;
                for (uint64_t p = s; p < s + we; p++) f += pres[c * n + p] == '1';
                if (s == 0 || f > w.best_found) { w.best_found = f; w.best_start = (uint32_t)s; }
                if (f >= thr) {
                    if (!w.windows_passing) w.first_start = (uint32_t)s;
                    w.last_start = (uint32_t)s;
                    w.windows_passing++;
                }
            }
            if (!w.windows_passing) continue;
            CHECK(at < hoff[i + 1] && col[at] == c && memcmp(&rec[at], &w, sizeof w) == 0, "sequence %d column %llu", i, (unsigned long long)c);
            at++;
        }
        CHECK(at == hoff[i + 1], "sequence %d has %llu hits too many", i, (unsigned long long)(hoff[i + 1] - at));
    }
    if (total) {
        std::fill(col.begin(), col.end(), 0xABABABABu);
        std::fill(hoff.begin(), hoff.end(), 0xABABABABABABABABull);
        CHECK(bigsi_cpu_window_search(ix, blob.data(), off.data(), 6, k, window, threshold, used.data(), need.data(), hoff.data(), col.data(), rec.data(), total - 1) == BIGSI_ERR_CAPACITY, "capacity");
        CHECK(hoff[6] == total && col[0] == 0xABABABABu, "the capacity protocol");
    }
    CHECK(bigsi_cpu_close(ix) == 0, "%s", bigsi_cpu_last_error());
}

int main()
{
    planners();
    for (uint64_t n_cols : {1ull, 63ull, 64ull, 65ull, 129ull})
        for (uint32_t window : {1u, 2u, 3u, 15u, 16u})
            for (double t : {1.0, 0.4}) twin(97, n_cols, 2, 5, window, t);
    printf("window planner and twin: ok\n");
    return 0;
}
