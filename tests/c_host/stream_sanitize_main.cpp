// A stand-alone program (its own main) that drives the cut rule of the streamed search (bigsi_amd/csrc/bigsi_launch.hpp:
// stream_limits, stream_chunk_end, stream_round_to_launches) over seeded offset arrays the way search_stream_impl does -- cut, round,
// move on -- and checks that the chunks tile [0, n_seqs) in order, that no chunk breaks a limit it could have kept, and that the
// functions read offsets[next .. end] and nothing behind offsets[n_seqs] (the arrays are exactly n_seqs + 1 entries on the heap).  Meant
// to be built with -fsanitize=address,undefined and run on the CPU: tests/test_stream_plan_host.py compiles and runs it.  Nothing
// sanitized is loaded into Python.
// Test infrastructure only: nothing in the product loads this file.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../bigsi_amd/csrc/bigsi_launch.hpp"

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

static uint64_t positions(const std::vector<uint64_t> &off, uint64_t i, uint32_t k)
{
    const uint64_t len = off[i + 1] - off[i];
    return len >= k ? len - k + 1 : 0;
}

// one stream over `off` (n_seqs + 1 entries, exactly): returns the number of chunks
static uint64_t stream(const std::vector<uint64_t> &off, uint32_t k, uint64_t limit_pos, uint64_t limit_seqs, uint32_t launch_q, bool exact)
{
    const uint64_t n_seqs = off.size() - 1;
    uint64_t next = 0, chunks = 0;
    while (next < n_seqs) {
        const bigsi::StreamChunk c = bigsi::stream_chunk_end(off.data(), n_seqs, next, k, limit_pos, limit_seqs);
        CHECK(!c.bad_offsets, "offsets refused at %llu", (unsigned long long)next);
        CHECK(c.end > next && c.end <= n_seqs && c.end - next <= limit_seqs, "chunk [%llu, %llu)", (unsigned long long)next, (unsigned long long)c.end);
        uint64_t pos = 0, raw = 0, max_pos = 0;
        for (uint64_t i = next; i < c.end; i++) {
            const uint64_t n = positions(off, i, k);
            pos += std::max<uint64_t>(n, 1);
            raw += n;
            max_pos = std::max(max_pos, n);
        }
        CHECK(pos == c.pos && max_pos == c.max_pos, "chunk at %llu: pos %llu, max_pos %llu", (unsigned long long)next, (unsigned long long)c.pos, (unsigned long long)c.max_pos);
        // over the limit only as a chunk of one; and it ended for a reason
        CHECK(c.end - next == 1 || raw <= limit_pos, "chunk at %llu holds %llu positions", (unsigned long long)next, (unsigned long long)raw);
        CHECK(c.end == n_seqs || c.end - next == limit_seqs || c.pos + positions(off, c.end, k) > limit_pos, "chunk at %llu ended early", (unsigned long long)next);
        const uint64_t n = bigsi::stream_round_to_launches(c.end - next, launch_q, c.end < n_seqs, exact, false);
        CHECK(n >= 1 && n <= c.end - next, "rounding of %llu gave %llu", (unsigned long long)(c.end - next), (unsigned long long)n);
        if (n != c.end - next) CHECK(exact && c.end < n_seqs && n % launch_q == 0 && c.end - next >= 2ull * launch_q && c.end - next - n < launch_q, "rounding %llu -> %llu", (unsigned long long)(c.end - next), (unsigned long long)n);
        CHECK(bigsi::stream_round_to_launches(c.end - next, launch_q, c.end < n_seqs, exact, true) == c.end - next, "a band chunk was rounded");
        next += n;
        chunks++;
    }
    CHECK(next == n_seqs, "the chunks end at %llu of %llu", (unsigned long long)next, (unsigned long long)n_seqs);
    return chunks;
}

int main()
{
    uint64_t total = 0;
    for (uint64_t n_seqs : {1ull, 2ull, 5ull, 64ull, 300ull, 5000ull})
        for (uint32_t k : {1u, 31u})
            for (uint64_t max_len : {0ull, 30ull, 40ull, 100ull, 5000ull})
                for (uint64_t limit_pos : {1ull, 70ull, 2000ull, 1ull << 20})
                    for (uint64_t limit_seqs : {1ull, 16ull, 4096ull})
                        for (uint32_t launch_q : {8u, 768u}) {
                            std::vector<uint64_t> off(n_seqs + 1, 0);
                            for (uint64_t i = 0; i < n_seqs; i++) off[i + 1] = off[i] + rnd() % (max_len + 1);
                            total += stream(off, k, limit_pos, limit_seqs, launch_q, true);
                            total += stream(off, k, limit_pos, limit_seqs, launch_q, false);
                        }
    // decreasing offsets: refused at the pair, nothing read behind it (the array ends right there)
    for (uint64_t bad : {0ull, 1ull, 7ull}) {
        std::vector<uint64_t> off(bad + 2);
        for (uint64_t i = 0; i <= bad; i++) off[i] = 100 * (i + 1);
        off[bad + 1] = off[bad] - 1;
        const bigsi::StreamChunk c = bigsi::stream_chunk_end(off.data(), bad + 1, 0, 31, 1ull << 20, 4096);
        CHECK(c.bad_offsets, "decreasing offsets at pair %llu accepted", (unsigned long long)bad);
    }
    // offsets near 2^64 and limits at the ends of their range
    {
        const uint64_t top = ~0ull;
        std::vector<uint64_t> off = {top - 300, top - 200, top - 100, top};
        CHECK(stream(off, 31, top, 4096, 8, true) == 1 && stream(off, 31, 0, 4096, 8, true) == 3, "offsets near 2^64");
    }
    for (double thr : {1.0, 0.4, 0.0})
        for (int scored = 0; scored < 2; scored++)
            for (int force = 0; force < 2; force++)
                for (uint64_t seqs : {0ull, 1ull, 4096ull, 4097ull, ~0ull}) {
                    bigsi::StreamOverrides o;
                    o.chunk_seqs = seqs;
                    const bigsi::StreamLimits l = bigsi::stream_limits(thr, scored != 0, force != 0, o);
                    CHECK(l.seqs >= 1 && l.seqs <= bigsi::kStreamChunkSeqs && l.chunk_pos() == (thr == 1.0 || scored ? l.small_pos : l.large_pos), "limits");
                    CHECK(l.band_chunks == (thr == 1.0 && !scored && !force), "band_chunks");
                }
    CHECK(total > 100000, "only %llu chunks", (unsigned long long)total);
    printf("stream cuts, rounding and limits: ok\n");
    return 0;
}
