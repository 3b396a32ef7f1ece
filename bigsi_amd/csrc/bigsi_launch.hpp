// bigsi_launch.hpp -- the launch rule of a batch run, host-only: how K1 goes out (k1_plan) and how the row-AND kernels
// (k_and_exact, k_and_count, k_count_combine) are launched for a batch of queries (plan_row_and), the sweep of the column popcounts
// (plan_col_popcount), the per-call tables of the column compaction (plan_compact_columns), the sweep of the row folding
// (plan_fold_rows), the sweep of the k-mer prevalence (plan_kmer_prevalence), the per-call tables, launch shape and destination
// window of the column collapse (plan_collapse_columns) and of the consensus collapse (plan_consensus_columns) and the chunks, slices,
// scratch and per-call tables of the pairwise popcounts (plan_pairwise, pairwise_tables) and the launch shape and stream cuts of the query-set
// tally (plan_tally, plan_tally_chunks; pinned by tests/c_host/tally_host.cpp and tests/test_tally_host.py) and what the exact k-mer
// counter decides about a call and its table (plan_kmer_count_add, kmer_stage_chunk, plan_kmer_table; pinned by
// tests/c_host/kmercount_plan_host.cpp and tests/test_kmercount_plan_host.py) and the segments, plane bucket, grid and refusals of the
// windowed search's sweep (plan_window_search; pinned by tests/c_host/window_host.cpp and tests/test_window_host.py) and the band sweep
// of a large exact batch (plan_band_sweep, band_window, band_lower_bound; pinned by tests/c_host/band_plan_host.cpp and
// tests/test_band_plan_host.py) and the chunk cuts of the streamed search (stream_limits, stream_chunk_end, stream_round_to_launches;
// pinned by tests/c_host/stream_plan_host.cpp and tests/test_stream_plan_host.py) and the launch shape of the hit-list compaction and
// the size of the pinned export (plan_hits, export_spec; pinned by tests/c_host/hits_plan_host.cpp and tests/test_hits_plan_host.py).
// Pure functions of a handful of integers
// (and, for the compaction, the collapses and the pairwise popcounts, of the keep bitmap / the group map / the column lists): no HIP,
// no batch, no index.  bigsi_hip.hip carries the plans out; tests/c_host/launch_host.cpp, compact_host.cpp, fold_host.cpp,
// prevalence_host.cpp, collapse_host.cpp, consensus_host.cpp and pairwise_host.cpp compile this header as plain host C++ and
// tests/test_abi_and_host.py, test_sample_stats_host.py, test_compact_columns_host.py, test_fold_rows_host.py,
// test_kmer_prevalence_host.py, test_collapse_columns_host.py, test_consensus_columns_host.py and test_pairwise_host.py pin the
// decisions on the CPU.
//
// Every constant below was measured on an MI355X; the notes beside them say against what.  A GPU test compares results, and a slip
// here keeps results right and costs the 3 to 20 % those notes record: change a constant only with a new measurement, and the pinned
// shapes of the CPU test with it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

static inline uint64_t round_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }
static inline uint64_t ceil_div(uint64_t x, uint64_t a) { return (x + a - 1) / a; }

namespace bigsi {

constexpr int kBlock = 256;      // 4 wavefronts
constexpr int kVec = 2;          // uint64 words per lane per row load (16 B/lane, 1 KiB per wave instruction)

// K1 fused (k_kmerize_lds): ONE launch for batches whose longest query has at most kLdsMaxPos k-mer positions (a 4 kbp query)
constexpr uint32_t kLdsMaxPos = 4096;

// ------------------------------------------------------------------------------ K1
enum K1Route { K1_ELEMENTS, K1_WAVE, K1_LDS, K1_GLOBAL };
struct K1Plan {
    K1Route route;
    uint32_t hs_cap = 0, sq_bytes = 0, tab_mult = 4, tab_cap = 2;
    size_t lds = 0;
};

// `max_pos` / `max_len`: k-mer positions / bytes of the batch's longest query; `elements`: the batch holds explicit k-mers
static inline K1Plan k1_plan(uint32_t n_seqs, uint64_t max_pos, uint64_t max_len, bool elements, bool force_global)
{
    K1Plan p;
    if (elements) { p.route = K1_ELEMENTS; return p; }
    if (!force_global && max_pos <= 64) { p.route = K1_WAVE; return p; }
    // dedupe table of the LDS route: 4 slots per position when that fits the LDS window (shorter probe chains), else 2
    p.hs_cap = (uint32_t)round_up(std::max<uint64_t>(max_pos, 1), 4);
    p.sq_bytes = (uint32_t)round_up(max_len + 16, 16);
    // (a handful of queries -- a latency-bound call -- have the LDS to themselves: 8 slots per position, insert phase of one 1 kbp
    // query 2.04 / 1.08 / 0.80 us at 2 / 4 / 8)
    p.tab_mult = n_seqs <= 32 ? 8u : 4u;
    for (;; p.tab_mult /= 2) {
        p.tab_cap = 2;
        while (p.tab_cap < p.tab_mult * max_pos && p.tab_cap < (1u << 30)) p.tab_cap <<= 1;
        p.lds = (size_t)(p.tab_cap + p.tab_cap / 32 + 4) * 4 + 64 + (size_t)p.hs_cap * 4 + 2 * p.sq_bytes;      // table (+ sort pad) | scan | fingerprints | sequence | its complement
        if (p.lds <= 60 * 1024 || p.tab_mult == 2) break;
    }
    // fused single-launch K1 (dedupe table + sequence in LDS) when every query fits the default 64 KiB dynamic-LDS window
    p.route = (!force_global && max_pos <= kLdsMaxPos && p.lds <= 60 * 1024) ? K1_LDS : K1_GLOBAL;
    return p;
}

// ------------------------------------------------------------------------------ row-AND
// The launch rule of a large exact batch (one slice, `blocks_per_q` workgroups per query of `wv`-word results): several launches, each
// a whole number of workgroups per CU (launches of 384 or 640 workgroups measured 0.72-0.78 of peak, 512 / 768 / 1024: 0.82-0.85) with
// about 1600-2000 LIVE wavefronts: all co-resident, sweeping the address-ordered row lists together, and no more bytes in flight than
// the memory system schedules well -- 10 M x 100 k (13 live wavefronts per query in 4 workgroups): 512 workgroups per launch 0.853 of
// peak, 1024: 0.819, 256: 0.68; a 12.5 k-sample shard (2 live wavefronts per workgroup): 1024 workgroups 0.773, 512: 0.581.  Queries
// per launch a multiple of 8 (the blockIdx -> XCD map).  A batch is cut only from two launches' worth of workgroups on.
struct ExactLaunch {
    uint64_t blocks;       // workgroups per launch
    uint32_t queries;      // queries per launch
};
static inline ExactLaunch exact_launch(uint64_t wv, uint64_t blocks_per_q)
{
    const uint64_t waves_per_q = ceil_div(wv, 64 * kVec);      // wavefronts of a query that hold columns
    const uint64_t kb = round_up(ceil_div((uint64_t)1600 * blocks_per_q, waves_per_q), 256);
    return {kb, (uint32_t)std::max<uint64_t>(8, (kb / blocks_per_q) / 8 * 8)};
}

// small batches: every query's row list is cut into this many slices so that ~2k wavefronts are in flight (see map_block); `waves`:
// wavefronts that hold columns in the whole batch
// (one 1 kbp query on 100 k samples, its slices spread over all XCDs (map_block): exact 35 / 14.7 / 16.6 / 22.9 us at
// 16 / 64 / 128 / 256 slices, counting 59 / 31 / 30 / 32 us; beyond that the atomics that combine the slices show)
// (counting, round 4: a slice of ~10 k-mers leaves 4 bit-sliced planes instead of 5 for k_count_combine to add up -- one
// 1 kbp query on 100 k samples at 0.4, the whole call: 60 slices 50.3 us, 96: 47.0, 128: 49.0; exact: 60 -> 36.3, 96 -> 35.8, 128 -> 41)
static inline uint32_t row_slices(uint64_t waves, uint64_t max_pos, bool exact)
{
    if (waves >= 1024) return 1;
    return (uint32_t)std::min<uint64_t>({exact ? 64u : 96u, ceil_div(2048, std::max<uint64_t>(waves, 1)), std::max<uint64_t>(max_pos / (exact ? 16 : 10), 1)});
}

// Queries per launch of a large exact batch in 256-thread workgroups on results of `wv` words: search_stream_impl cuts its chunks
// at whole launches (bigsi_exact_launch_queries)
static inline uint32_t exact_launch_queries(uint64_t wv)
{
    if (wv == 0) return 8;
    return exact_launch(wv, ceil_div(wv, (uint64_t)256 * kVec)).queries;
}

// what the rule reads of a batch, its index and its run
struct RowAndInput {
    uint32_t n_seqs;
    uint64_t wv;                // 64-column words of a result vector
    uint64_t max_pos;           // k-mer positions of the longest query
    uint32_t h;                 // rows per k-mer
    bool exact;                 // k_and_exact (threshold 1.0), else the counting kernels
    bool no_sort, early_exit, sparse_counts;      // BIGSI_RUN_NO_SORT / _EARLY_EXIT / _SPARSE_COUNTS
};

// one row-AND launch over the queries [q0, q1)
struct RowAndLaunch {
    uint32_t q0, q1;
    uint64_t grid;              // workgroups
    uint32_t block;             // threads per workgroup: 64, 128 or 256
    uint32_t tiles;             // column tiles (workgroups) per query and slice
    uint32_t slices;
    uint32_t unroll;            // row loads a lane keeps in flight, k_and_exact<unroll>: 4 or 8 (the counting kernels do not read it: 8)
    bool needs_preset;          // exact, sliced: the slices AND into the launch's result words, which start as all ones
};

struct RowAndPlan {
    uint64_t too_large = 0;     // > 0: the batch does not fit one launch (this many workgroups) and the plan has no launches
    uint32_t slices = 1;        // of the whole batch (a chunked batch's last launch may differ: launch())
    bool want_sorted = false;   // K2 reads an address-ordered copy of the row lists (K1's LDS route or k_sort_rows makes it)
    bool preset = false;        // exact, sliced: ALL result words start as all ones -- K1 sets them on its way, or a memset does
    int P = 6;                  // counter planes: 6, 10, 12, 16 or 32
    uint32_t count_bytes = 2;   // of a counter
    uint32_t planes_out = 0;    // counting, sliced: planes of a slice's partial counts
    bool combine = false;       // counting, sliced: k_count_combine adds the slices up ...
    uint64_t combine_grid = 0;  // ... in this many workgroups of kBlock threads
    bool deep = false;          // counting: the software-pipelined kernel variant (it exists for h = 3 and 4)
    bool early = false;         // counting: early exit (never together with `deep`)
    uint32_t n_launches = 0;

    RowAndLaunch launch(uint32_t i) const;

    // the whole batch's shape, and what launch() needs
    RowAndInput in{};
    uint32_t block = 256, tiles = 1, chunk_q = 0;
};

// Workgroups of a launch of `n` queries.  Sliced launches map workgroups to queries in plain order -- map_block -- and need no padding
// to 8 queries: a single sliced query used to launch 8 x its workgroups, seven eighths of them leaving at once.
static inline uint64_t row_and_grid(uint64_t n, uint64_t tiles, uint64_t slices)
{
    return (slices > 1 ? n : ceil_div(n, 8) * 8) * tiles * slices;
}

// One-wavefront workgroups for `n` unsliced queries?  Batches of a few thousand wavefronts (80 ... 300 gene-length queries on
// 100 k samples) are a single launch, a CU's share of it is what bounds it, and 4-wavefront workgroups leave the CUs unevenly loaded
// (320 / 576 / 800 workgroups on 256 CUs: 0.69 / 0.68 / 0.71 of peak against 0.81 / 0.76 / 0.76 with 64 threads); the large
// launches, sized in whole workgroups per CU, keep 256 threads (0.85 against 0.79).  Nor is a launch that already is a whole number of
// 4-wavefront workgroups per CU "mid" (256 queries on a 62.5 k-sample shard: 512 workgroups, 0.80-0.82 either way).
static inline bool mid_launch(uint64_t n, uint64_t wv, uint64_t waves)
{
    return waves >= 1024 && row_and_grid(n, ceil_div(wv, 256 * kVec), 1) % 256 != 0;
}

static inline RowAndPlan plan_row_and(const RowAndInput &in)
{
    RowAndPlan p;
    p.in = in;
    const uint64_t waves_per_q = ceil_div(in.wv, 64 * kVec), all_waves = in.n_seqs * waves_per_q;
    // caller-owned result vectors (a shard's slot of a gather buffer) can be preset and sliced like the batch's own (the counting
    // path then cuts its hit mask from the slices' summed partial counts, k_count_combine)
    p.slices = row_slices(all_waves, in.max_pos, in.exact);
    const bool few = all_waves < 1024;
    // K1e: address-ordered copy of the row lists for K2
    // exact path only: there every row can move freely (+4.7 % C3, +7.6 % C4-shard, interleaved A/B); on the counting path a
    // k-mer's h rows must stay together and ordering k-mers by their first row measured 1.00x
    // and only for long row lists (>= 1024 rows per query): for read-length queries (C2: 93 rows) the extra launch costs more
    // than the ordering gains (0.100 vs 0.083 ms per step measured)
    // (not for the few queries of a latency-bound call either: their row lists are cut into slices over many workgroups and the
    // ordering buys nothing, it only lengthens the chain of kernels: 10 us of a 65 us single query)
    p.want_sorted = in.exact && !few && !in.no_sort && in.max_pos * in.h >= 1024;
    // planes needed for the largest possible count = max k-mers of any sequence in the batch
    const uint64_t maxu = in.max_pos;
    p.P = maxu < (1ull << 6) ? 6 : maxu < (1ull << 10) ? 10 : maxu < (1ull << 12) ? 12 : maxu < (1ull << 16) ? 16 : 32;
    p.count_bytes = p.P <= 16 ? 2 : 4;
    p.preset = p.slices > 1 && in.exact;

    // the counting kernels are compiled for at most 256 threads per workgroup (register budget of the plane arrays)
    // one-wavefront workgroups: see mid_launch
    // (exact batches large enough for exact_launch to cut them -- from 256 such queries on -- are not "mid")
    const uint64_t t256 = ceil_div(in.wv, 256 * kVec);
    const bool mid = all_waves < 4096 && mid_launch(in.n_seqs, in.wv, all_waves) &&
                     !(in.exact && row_and_grid(in.n_seqs, t256, 1) >= 2 * exact_launch(in.wv, t256).blocks);
    // (a sliced exact launch -- a latency-bound call -- in workgroups of two wavefronts: the pieces spread more evenly over the CUs and the
    // stragglers end sooner; one 1 kbp query on 100 k samples, the call: 256 -> 41.9, 128 -> 41.2, 64 -> 41.4 us; counting: no difference)
    p.block = mid ? 64 : p.preset ? 128 : 256;
    p.tiles = (uint32_t)ceil_div(in.wv, (uint64_t)p.block * kVec);

    // (the bound counts the queries padded to 8, sliced or not)
    const uint64_t total_blocks = row_and_grid(in.n_seqs, (uint64_t)p.tiles * p.slices, 1);
    if (total_blocks > 0x7FFFFFFFull) { p.too_large = total_blocks; return p; }
    // large exact batches go out as several launches (exact_launch); the counting kernel measured -4 ... 0 % chunked and stays one launch
    p.chunk_q = in.n_seqs;
    if (p.slices == 1 && in.exact) {
        const ExactLaunch el = exact_launch(in.wv, p.tiles);
        if (total_blocks >= 2 * el.blocks) p.chunk_q = el.queries;
    }
    p.n_launches = p.chunk_q ? (uint32_t)ceil_div(in.n_seqs, p.chunk_q) : 0;

    if (!in.exact) {
        // a sliced (small) batch: every slice leaves its partial counts bit-sliced in scratch memory -- as many planes as a slice's
        // k-mers need -- and k_count_combine adds them up, thresholds and expands (no presets, no atomics)
        if (p.slices > 1) {
            const uint64_t per_slice = ceil_div(std::max<uint64_t>(in.max_pos, 1), p.slices);
            while (p.planes_out < (uint32_t)p.P && (per_slice >> p.planes_out) != 0) p.planes_out++;
            p.combine = true;
            p.combine_grid = in.n_seqs * ceil_div(in.wv, kBlock / 8);      // 32 words per workgroup, 8 slice groups per word
        }
        p.early = in.early_exit && in.sparse_counts && p.slices == 1;
        // fewer than ~3 wavefronts per SIMD in the whole grid (e.g. 128 gene-length queries): the software-pipelined loop,
        // whose wavefronts load the next k-mers' rows while adding the current ones (5.6 -> 6.3 TB/s at 128 x 2-4 kbp; with a
        // full grid other wavefronts already cover the ALU phase and it measured -2 ... +0 %)
        const uint64_t grid_waves = (uint64_t)in.n_seqs * p.tiles * (p.block / 64);
        // (only with >= 12 planes, i.e. queries of >= 1024 k-mers: at 10 planes the ALU phase is short and it measured -2 %)
        p.deep = p.slices == 1 && p.P >= 12 && grid_waves < 3 * 1024 && !p.early;
    }
    return p;
}

inline RowAndLaunch RowAndPlan::launch(uint32_t i) const
{
    RowAndLaunch l;
    l.q0 = i * chunk_q;
    l.q1 = (uint32_t)std::min<uint64_t>((uint64_t)l.q0 + chunk_q, in.n_seqs);
    l.block = block;
    l.tiles = tiles;
    l.slices = slices;
    const uint32_t n = l.q1 - l.q0;
    if (chunk_q < in.n_seqs && n < chunk_q && block == 256) {
        // the last launch of a batch that is not a multiple of the launch size is a batch of its own kind: with a few thousand
        // wavefronts one-wavefront workgroups (mid_launch), with fewer the sliced launch of a small batch.  The rule of a whole
        // batch, except that
        //  - a sliced tail keeps the workgroups of 256 threads its batch runs in (a whole batch: 128);
        //  - a tail has no upper bound of 4096 wavefronts (it has fewer than a launch's 1600-2000 anyway, unless its rows are
        //    wider than 4 M columns, when a launch is the minimum of 8 queries).
        const uint64_t waves = (uint64_t)n * ceil_div(in.wv, 64 * kVec);
        if (waves < 1024) l.slices = row_slices(waves, in.max_pos, true);
        else if (mid_launch(n, in.wv, waves)) {
            l.block = 64;
            l.tiles = (uint32_t)ceil_div(in.wv, 64 * kVec);
        }
    }
    l.grid = row_and_grid(n, l.tiles, l.slices);
    l.needs_preset = in.exact && l.slices > 1;
    // row loads a lane keeps in flight: 8, or 4 when 8 would put more bytes in flight on the chip (queries of the launch x row bytes x
    // loads) than the memory system schedules well -- the optimum measured at 8-13 MB.  Interleaved A/B: 256 queries per launch on
    // 62.5 k-sample shards (7.8 KB rows: 16 MB at 8 loads): 4 -> +3.3 % (C4 shard 263 -> 272 M lookups/s) / +2.2 % (north-star shard),
    // 6 -> +1.5 %, 2 -> -17 %; unchunked C3 launches of 160-248 queries (16-25 MB): 4 -> +2 ... +9 %.  At 12.8 MB 8 stays: C3's 128-query
    // launches (4: -5 %) and C3 split over 2 / 4 / 8 GPUs -- 256 x 6.3 KB, 512 x 3.1 KB, 1024 x 1.6 KB rows per launch (4: -7 / -10 /
    // -7 %).
    const uint64_t in_flight_at_8 = (uint64_t)n * in.wv * 8 * 8;
    l.unroll = (in.exact && in_flight_at_8 > (29ull << 19) /* 14.5 MB */ && l.slices == 1) ? 4 : 8;
    return l;
}

// ------------------------------------------------------------------------------ band sweep (k_and_exact_band)
// A large exact batch references its index's rows several times over (rho = n_seqs x max_pos x h / m references per row: 4096 queries
// of 1 kbp at h = 4 on 10 M rows 1.59, half of the references repeats of a row some other query holds too).  plan_row_and's launches
// hold ~128 queries x all segments, and two queries that share a row meet it a launch apart, from HBM both times.  The band sweep turns
// the loops round: a launch is ONE 1 KiB column segment (a band) of EVERY query of the batch, a wavefront per query, all of them
// sweeping their address-ordered lists low -> high together, so that the second reference to a row comes while its lines are still in
// the caches behind the CUs.  Optionally a band is cut into address windows, a launch each: the wavefront finds its part of the list
// by binary search and carries its accumulator from window to window through the result words (one owner per word, launches
// stream-ordered: plain load and store).
//
// Measured with the bare probe (scripts/probe/row_probe.hip, mode shared; profiles/band_sweep_probe.txt; 125 GB matrix of 12.5 KB rows,
// lists of 3880 rows, GB/s = references x 1 KiB / time; `sorted` in the same job 6494-6501, with scalar row-id loads 6618-6664):
//   - plain loads see the repeats, non-temporal loads do not: 4096 wavefronts, rho 1.59, one window, 2 loads: plain 7467, NT 6756
//     (NT with NO repeats: 6753).  Without repeats plain loads are the slower ones (6113): the route pays only where rows repeat.
//   - loads in flight per lane 2 / 4 / 8 (4096 wavefronts, rho 1.59, one window): 7467 / 7214 / 6638          -> kBandUnroll = 2
//   - windows 1 / 4 / 16 / 64, 4096 wavefronts: 7467 / 7297 / 6857 / 5593; 8192 wavefronts (repeated share 0.70):
//     6814 / 7192 / 7128 / 6428                                  -> one window up to 4096 queries, kBandWindowsLarge = 4 beyond
//   - two segments per launch (8192 wavefronts for 4096 queries): 6539 at one window, 6929 at 16            -> kBandSegs = 1
//   - repeated share 0 / 0.50 / 0.70 (rho 0 / 1.59 / 3.18, 4096 wavefronts): 6113 / 7467 / 7753.  Between the first two the rate
//     crosses k_and_exact's 6.8 TB/s near a share of 0.26 (rho 0.63) -- interpolated, not measured -- and the route is taken from
//     kBandMinRho = 1.0 on (share 0.37), where the interpolated rate is 4 % above it.
//   - wavefronts per launch (one window, 2 loads, rho 1.59 / 3.18): 512: 1831 / 1917, 1024: 3527 / 3758, 2048: 6113 / 6591,
//     3072: 7563 / 7907, 4096: 7467 / 7753 -- with two loads in flight a launch needs some 3000 wavefronts to fill the memory system,
//     and below that plan_row_and's launches (13 segments x 8 loads of 128 queries) are the faster ones     -> kBandMinQueries = 3072
//   - bytes in flight: the largest launch measured is 8192 wavefronts x 2 loads x 1 KiB = 16 MiB = kBandInFlightCap; larger batches
//     keep plan_row_and's launches.
//   - a last segment that holds few columns costs a launch nearly as long as a full one (its wavefronts wait for as many rows): the
//     27 words of C3's 13th segment (1563 result words) as a launch of their own against riding in the 12th segment's launch (8192
//     wavefronts, 14 lanes of every second one live), bench.py's step, interleaved on one box: 56.72 / 57.33 / 57.38 ms against
//     55.33 / 55.91 / 56.01.  Taken up to kBandTailWords = 32 words (a quarter segment; only 27 was measured).
// The blockIdx -> XCD map of k_and_exact is not kept: a wavefront is a (query, segment) and the probe ran without it.
constexpr uint32_t kBandUnroll = 2;
constexpr uint32_t kBandSegs = 1;
constexpr uint32_t kBandWindowsLarge = 4;
constexpr uint32_t kBandOneWindowQueries = 4096;
constexpr double kBandMinRho = 1.0;
constexpr uint32_t kBandMinQueries = 3072;
constexpr uint64_t kBandInFlightCap = 16ull << 20;
constexpr uint32_t kBandMaxWindows = 1u << 16;
constexpr uint64_t kBandTailWords = 32;

// The address-ordered lists are bucket-sorted, not fully sorted: ascending in (row id >> shift), any order inside a bucket, with the
// smallest shift that leaves at most `buckets` buckets over [0, m) (k_sort_rows: kSortBuckets; K1's LDS route: its table's slots).
static inline uint32_t sort_shift(uint64_t m, uint64_t buckets)
{
    uint32_t shift = 0;
    while (m && ((m - 1) >> shift) >= buckets) shift++;
    return shift;
}

// threads of k_sort_rows' workgroup (its two instances): 1024 per query for long row lists (a 1 kbp query at h = 4 has 3880 rows),
// kBlock otherwise (pinned, with k1_plan's routes, by tests/c_host/launch_host.cpp and tests/test_knockout_host.py)
static inline uint32_t sort_rows_block(uint64_t max_pos, uint32_t h) { return max_pos * h >= 2048 ? 1024u : (uint32_t)kBlock; }

// rows [lo, hi) of window w of W over m rows, cut at whole sort buckets (so that a window is a contiguous piece of every list): the
// windows partition [0, m) for every W >= 1 (W above the number of buckets: most are empty)
struct BandWindow {
    uint64_t lo, hi;
};
static inline BandWindow band_window(uint64_t m, uint32_t w, uint32_t W, uint32_t shift)
{
    const uint64_t nb = m ? ((m - 1) >> shift) + 1 : 0;
    const uint64_t lo = (uint64_t)((unsigned __int128)nb * w / W) << shift, hi = (uint64_t)((unsigned __int128)nb * (w + 1) / W) << shift;
    return {std::min(lo, m), std::min(hi, m)};
}

// first index in the list r[0, n) whose row id is >= key, for a list ascending in (row id >> shift) and a key that is a multiple of
// 2^shift or the number of rows (a window bound).  The kernel runs the same loop on scalar loads: at most 17 steps for 2^17 rows
static inline uint64_t band_lower_bound(const uint64_t *r, uint64_t n, uint64_t key)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (r[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct BandLaunch {
    uint32_t seg0, nseg;        // the launch's segments [seg0, seg0 + nseg) (the last group may reach past the result's last segment)
    uint32_t window;            // of BandSweepPlan::windows
    uint64_t grid;              // workgroups of kBlock threads: a wavefront per (query, segment)
    uint32_t unroll;
};
struct BandSweepPlan {
    bool taken = false;
    uint32_t windows = 0, segs_per_launch = 0, seg_groups = 0, unroll = kBandUnroll;
    uint64_t grid = 0, in_flight = 0;      // of a launch: workgroups, bytes in flight (wavefronts x unroll x 1 KiB)
    uint32_t n_launches = 0;               // seg_groups x windows: group by group, a group's windows in ascending order
    bool merge_tail = false;               // the last group is the last TWO segments (kBandTailWords)
    BandLaunch launch(uint32_t i) const
    {
        const uint32_t g = i / windows;
        const bool tail = merge_tail && g + 1 == seg_groups;
        return {g * segs_per_launch, tail ? 2u : segs_per_launch, i % windows, tail ? 2 * grid : grid, unroll};
    }
};

// `forced` (BIGSI_RUN_BAND_SWEEP): whatever rho and the batch's size; forced_windows / forced_segs (bigsi_hip_band_set_limits): 0
// keeps the rule's value
static inline BandSweepPlan plan_band_sweep(const RowAndInput &in, uint64_t m, bool forced = false, uint32_t forced_windows = 0,
                                            uint32_t forced_segs = 0)
{
    BandSweepPlan p;
    if (!in.exact || in.early_exit || in.no_sort || in.n_seqs == 0 || in.wv == 0 || m == 0) return p;
    p.windows = forced_windows ? std::min(forced_windows, kBandMaxWindows) : in.n_seqs <= kBandOneWindowQueries ? 1 : kBandWindowsLarge;
    p.segs_per_launch = forced_segs ? std::min(forced_segs, 2u) : kBandSegs;
    const uint64_t segs = ceil_div(in.wv, 64 * kVec), waves = (uint64_t)in.n_seqs * p.segs_per_launch;
    p.seg_groups = (uint32_t)ceil_div(segs, p.segs_per_launch);
    p.grid = ceil_div(waves, kBlock / 64);
    p.in_flight = waves * p.unroll * 1024;
    if (p.grid > 0x7FFFFFFFull || (uint64_t)p.seg_groups * p.windows > 0x7FFFFFFFull) return p;
    if (!forced) {
        const RowAndPlan rp = plan_row_and(in);
        const double rho = (double)in.n_seqs * (double)in.max_pos * in.h / (double)m;
        if (rp.slices != 1 || !rp.want_sorted || rho < kBandMinRho || in.n_seqs < kBandMinQueries || p.in_flight > kBandInFlightCap) return p;
    }
    // a nearly empty last segment rides with its neighbour (one-window plans with the rule's own segments only)
    if (!forced_segs && p.windows == 1 && segs >= 2 && in.wv - (segs - 1) * 64 * kVec <= kBandTailWords && 2 * p.in_flight <= kBandInFlightCap) {
        p.merge_tail = true;
        p.seg_groups--;
    }
    p.n_launches = p.seg_groups * p.windows;
    p.taken = true;
    return p;
}

// ------------------------------------------------------------------------------ column popcounts (k_col_popcount, k_col_popcount_sum)
// The vertical popcount sweeps the whole matrix once: a wavefront owns one 1 KiB column segment (kVec words per lane) of a contiguous
// block of rows, adds the rows kColPopLoads at a time -- that many independent 16-byte loads in flight per lane, as k_and_exact<8>,
// reduced by a carry-save tree -- into kColPopPlanes bit-sliced planes, and flushes the planes into its own 32-bit counters (its slice
// of a [row block][column] scratch array) before they can overflow: kColPopPlanes planes hold 2^planes - 1 rows, so a flush is due
// every flush_groups groups of loads.  k_col_popcount_sum then adds the row blocks of a column up in 64 bits.
//   - Row blocks supply the parallelism: a 100 k-sample index has 13 column segments, a 62.5 k-sample shard 62, and the sweep wants
//     about kColPopWaves wavefronts whatever the width, so rows_per_block = rows x segments / kColPopWaves, in whole flush periods:
//     kColPopFlushRows = 960 rows (<= 2^planes - 1, a multiple of the 64 rows of a mask word and of kColPopLoads), so that every flush
//     of an unmasked sweep but a block's last carries a full period, and at least two periods.  A flush writes the wavefront's 32 KiB of
//     counters and every flush but its first reads them back first, the sum reads them once: 64 KiB per 960 KiB of rows, 6.7 % of the
//     sweep's traffic in the steady state and no more for a minimum block.
//   - Narrow indexes (fewer than four segments) run one-, two- or three-wavefront workgroups instead of idling wavefronts of four.
//   - No counter wraps: a wavefront's 32-bit counters see at most rows_per_block <= 2^31 rows (the rule raises the number of row
//     blocks beyond that), the sum is 64 bits wide.
constexpr int kColPopLoads = 8;
constexpr int kColPopPlanes = 10;
constexpr uint64_t kColPopWaves = 4096;
constexpr uint64_t kColPopFlushRows = 960;
static_assert(kColPopFlushRows % 64 == 0 && kColPopFlushRows % kColPopLoads == 0 && kColPopFlushRows < (1ull << kColPopPlanes), "a flush period is whole mask words and whole groups of loads, and fits the planes");
struct ColPopPlan {
    uint32_t block = 64;            // threads per workgroup: 64 per segment it covers, at most kBlock
    uint64_t seg_groups = 0;        // workgroups per row block
    uint64_t rows_per_block = 0;    // a multiple of kColPopFlushRows, hence of 64
    uint64_t row_blocks = 0;
    uint64_t grid = 0;              // seg_groups x row_blocks workgroups
    uint32_t flush_groups = 0;      // groups of kColPopLoads rows between two flushes
    uint64_t partial_stride = 0;    // 32-bit counters of one row block in the scratch array: stride_words x 64
};
static inline ColPopPlan plan_col_popcount(uint64_t num_rows, uint64_t stride_words)
{
    ColPopPlan p;
    const uint64_t segs = std::max<uint64_t>(ceil_div(stride_words, 64 * kVec), 1);
    p.block = (uint32_t)std::min<uint64_t>(segs, kBlock / 64) * 64;
    p.seg_groups = ceil_div(segs, p.block / 64);
    const uint64_t want_blocks = std::max<uint64_t>(kColPopWaves / segs, 1);
    p.rows_per_block = round_up(std::max<uint64_t>(ceil_div(num_rows, want_blocks), 2 * kColPopFlushRows), kColPopFlushRows);
    p.rows_per_block = std::min<uint64_t>(p.rows_per_block, (1ull << 31) / kColPopFlushRows * kColPopFlushRows);
    p.row_blocks = std::max<uint64_t>(ceil_div(num_rows, p.rows_per_block), 1);
    p.grid = p.seg_groups * p.row_blocks;
    p.flush_groups = (uint32_t)(kColPopFlushRows / kColPopLoads);
    p.partial_stride = stride_words * 64;
    return p;
}

// ------------------------------------------------------------------------------ column compaction (k_compact_columns)
// "Keep these columns, in order, and close the gaps": with K = popcount(keep) the j-th kept column of every row becomes column j.
// The keep mask is the same for all rows, so everything that depends on it alone is worked out HERE, once per call, and the kernel's
// hot loop is table-driven.  In plain column order (by_column: bit c of word w = column 64 w + c)
//   - a source word s is compressed to its kept bits -- a software pext, the parallel-suffix network of Hacker's Delight 7-4, whose
//     six move masks depend on the mask only: words[s].mv.  The device does x &= mask, then six times t = x & mv[i];
//     x = (x ^ t) | (t >> (1 << i));
//   - those bits are the kept columns of rank [before, before + popcount(mask)): they land in destination word before / 64 at bit
//     before % 64 and spill into the next one;
//   - a destination word o is the OR of the source words first_src[o] .. first_src[o + 1] (both included: a word on the boundary
//     feeds two), each shifted to its place.  first_src[o] = the first source word that holds a kept column of rank >= 64 o; the
//     entry behind the last one is the last source word that keeps a column.  first_src[o] >= o: compaction only moves bits towards lower columns,
//     which is what makes the kernel correct in place (see there).
// Bits of `keep` at columns >= num_cols are ignored.  Table sizes: 64 bytes per source word and 4 per destination word -- 100 KB for
// 100 k columns (it stays in the L2 of every XCD), 4 GiB at the ABI's 2^32 - 1 columns.
// Launch shape: a wavefront owns kCompactRows whole rows at a time (the tables' entries are loaded once for all of them, and the rows'
// loads are independent: that many 8-byte loads in flight per lane) and strides over the row groups; about kColPopWaves wavefronts
// whatever the shape, fewer wavefronts per workgroup for a handful of rows.
constexpr int kCompactRows = 8;
struct CompactWord {            // per source word, 64 bytes
    uint64_t mask;              // kept columns of the word, in plain column order
    uint64_t mv[6];             // move masks of the compress network (unused when mask is all ones or zero)
    uint32_t before;            // kept columns in front of this word
    uint32_t count;             // popcount(mask)
};
static_assert(sizeof(CompactWord) == 64, "k_compact_columns loads a table entry as four 16-byte pieces");
struct CompactPlan {
    uint64_t src_words = 0;     // ceil(num_cols / 64)
    uint64_t kept = 0;          // K
    uint64_t dst_words = 0;     // ceil(K / 64)
    std::vector<CompactWord> words;       // src_words entries
    std::vector<uint32_t> first_src;      // dst_words + 1 entries
    uint32_t block = 64;        // threads per workgroup: 64 per row group it covers at once, at most kBlock
    uint64_t grid = 0;          // workgroups; the wavefronts stride over the row groups
};
// software pext with a plan's move masks: what the device does per word (the CPU test drives it against naive selection)
static inline uint64_t compact_word(uint64_t x, const CompactWord &w)
{
    x &= w.mask;
    for (int i = 0; i < 6; i++) {
        const uint64_t t = x & w.mv[i];
        x = (x ^ t) | (t >> (1u << i));
    }
    return x;
}
// K alone, for a caller that has nothing to do when every column is kept
static inline uint64_t count_kept_columns(uint64_t num_cols, const uint8_t *keep)
{
    uint64_t k = 0;
    for (uint64_t b = 0; b < num_cols / 8; b++) k += (uint64_t)__builtin_popcount(keep[b]);
    if (num_cols & 7) k += (uint64_t)__builtin_popcount(keep[num_cols / 8] & (0xFF00u >> (num_cols & 7)) & 0xFFu);
    return k;
}
// `keep`: ceil(num_cols / 8) bytes in the row format (column c at byte c / 8 under 0x80 >> (c % 8))
static inline CompactPlan plan_compact_columns(uint64_t num_cols, const uint8_t *keep, uint64_t num_rows)
{
    CompactPlan p;
    p.src_words = ceil_div(num_cols, 64);
    p.words.resize(p.src_words);
    uint64_t before = 0;
    for (uint64_t s = 0; s < p.src_words; s++) {
        CompactWord &w = p.words[s];
        uint64_t m = 0;
        for (uint64_t c = s * 64; c < std::min(num_cols, s * 64 + 64); c++)
            if (keep[c >> 3] & (0x80u >> (c & 7))) m |= 1ull << (c & 63);
        w.mask = m;
        w.before = (uint32_t)before;
        w.count = (uint32_t)__builtin_popcountll(m);
        // Hacker's Delight 7-4: mk = the bits that have a dropped bit somewhere below them are counted by prefix XORs; mv[i] = the
        // kept bits that move down by 2^i in step i
        uint64_t mk = ~m << 1;
        for (int i = 0; i < 6; i++) {
            uint64_t mp = mk ^ (mk << 1);
            mp ^= mp << 2;
            mp ^= mp << 4;
            mp ^= mp << 8;
            mp ^= mp << 16;
            mp ^= mp << 32;
            const uint64_t mv = mp & m;
            w.mv[i] = mv;
            m = (m ^ mv) | (mv >> (1u << i));
            mk &= ~mp;
        }
        before += w.count;
    }
    p.kept = before;
    p.dst_words = ceil_div(p.kept, 64);
    // (the entry behind the last destination word: the last source word that keeps anything -- trailing words with empty masks feed
    // nobody and are not walked)
    uint64_t last = 0;
    for (uint64_t s = 0; s < p.src_words; s++)
        if (p.words[s].count) last = s;
    p.first_src.assign(p.dst_words + 1, (uint32_t)last);
    uint64_t o = 0;
    for (uint64_t s = 0; s < p.src_words && o < p.dst_words; s++)
        while (o < p.dst_words && (uint64_t)p.words[s].before + p.words[s].count > o * 64) p.first_src[o++] = (uint32_t)s;
    const uint64_t groups = std::max<uint64_t>(ceil_div(num_rows, kCompactRows), 1);
    p.block = (uint32_t)std::min<uint64_t>(groups, kBlock / 64) * 64;
    p.grid = std::min<uint64_t>(ceil_div(groups, p.block / 64), kColPopWaves / (kBlock / 64));
    return p;
}

// ------------------------------------------------------------------------------ row folding (k_fold_rows)
// Destination row r = the OR of the source rows r, r + m', ..., r + (factor - 1) m' (m' = m_dst = m / factor): the matrix of the same
// samples under a Bloom filter of m' bits.  One streaming pass, decomposed as the column popcounts: a wavefront owns one 1 KiB column
// segment (kVec words per lane) of a contiguous block of DESTINATION rows, the grid is segments x row blocks.
//   - Loads in flight: a step of the kernel takes rows_per_step destination rows at once, rows_per_step x factor independent 16-byte
//     loads per lane, for factor < kFoldLoads (ceil(kFoldLoads / factor) rows: 8 to 14 loads); for factor >= kFoldLoads it takes one
//     destination row and its source rows in groups of kFoldLoads, ORed into a running value.
//     INVARIANT (the kernel's register budget): rows_per_step x min(factor, kFoldLoads) <= kFoldMaxLoads = 16 loads of 4 VGPRs each,
//     64 VGPRs of row data per lane; the kernel's arrays are sized by it and tests/test_fold_rows_host.py checks it for every plan.
//   - Row blocks: about kFoldWaves wavefronts whatever the shape.  The figure is INHERITED from the column popcounts' sweep
//     (kColPopWaves, measured there), not measured for this kernel.  A block is a whole number of steps, and at least kFoldMinRows
//     rows (a wavefront that folds fewer has more launch than work), so only a matrix of fewer than kFoldMinRows x (wanted blocks) rows
//     runs fewer wavefronts.  No block is empty: row_blocks = ceil(m_dst / rows_per_block), the last one is ragged.
//   - The grid is seg_groups x row_blocks <= max(2^17, 4 x kFoldWaves) workgroups for any stride the ABI allows (2^32 - 1 columns
//     = 2^26 words = 2^19 segments): it fits 31 bits.
constexpr int kFoldLoads = 8;
constexpr int kFoldMaxLoads = 16;
constexpr uint64_t kFoldWaves = kColPopWaves;
constexpr uint64_t kFoldMinRows = 64;
struct FoldPlan {
    uint32_t block = 64;            // threads per workgroup: 64 per segment it covers, at most kBlock
    uint64_t seg_groups = 0;        // workgroups per row block
    uint32_t rows_per_step = 1;     // destination rows a lane folds at once
    uint64_t rows_per_block = 0;    // a multiple of rows_per_step
    uint64_t row_blocks = 0;
    uint64_t grid = 0;              // seg_groups x row_blocks workgroups
};
static inline uint32_t fold_rows_per_step(uint64_t factor)
{
    return factor >= (uint64_t)kFoldLoads ? 1u : (uint32_t)ceil_div(kFoldLoads, std::max<uint64_t>(factor, 1));
}
// `stride_words`: the DESTINATION's row stride (every word of it is written)
static inline FoldPlan plan_fold_rows(uint64_t m_dst, uint64_t factor, uint64_t stride_words)
{
    FoldPlan p;
    const uint64_t segs = std::max<uint64_t>(ceil_div(stride_words, 64 * kVec), 1);
    p.block = (uint32_t)std::min<uint64_t>(segs, kBlock / 64) * 64;
    p.seg_groups = ceil_div(segs, p.block / 64);
    p.rows_per_step = fold_rows_per_step(factor);
    const uint64_t want_blocks = std::max<uint64_t>(kFoldWaves / segs, 1);
    p.rows_per_block = round_up(std::max<uint64_t>(ceil_div(m_dst, want_blocks), kFoldMinRows), p.rows_per_step);
    p.row_blocks = std::max<uint64_t>(ceil_div(m_dst, p.rows_per_block), 1);
    p.grid = p.seg_groups * p.row_blocks;
    return p;
}

// ------------------------------------------------------------------------------ k-mer prevalence (k_kmer_prevalence)
// For every unique k-mer of a batch the popcount of the AND of its h rows over the whole width (under a mask): the horizontal twin of
// the column popcounts.  A work item is (slot, slice): a slot is a k-mer position of the batch (slot t of sequence q is a unique
// k-mer iff t - pos_off[q] < num_unique[q]; the others cost their test), a slice a run of segs_per_slice 1 KiB column segments.  A
// wavefront owns one slice and strides over the slots; a lane owns kVec words of a segment.
//   - Slices: one per k-mer once the batch has kPrevWaves unique k-mers; fewer k-mers are cut into enough slices to reach that many
//     items, never more than there are segments (one 1 kbp query on 13 segments: 5 slices).  No slice is empty:
//     slices = ceil(segs / segs_per_slice), the last one is ragged.  A one-segment index has one slice.
//   - Wavefronts: about kPrevWaves.  The figure is INHERITED from the column popcounts' sweep (kColPopWaves, measured there), not
//     measured for this kernel.  A batch whose slots are at most twice the wavefronts of a slice gets one wavefront per slot (at most
//     2 x kPrevWaves in all: striding would leave half of them a second slot while the others are done).
//   - Loads in flight: a step takes segs_per_step segments x the k-mer's rows for h < kPrevLoads (ceil(kPrevLoads / h) segments: 8 to
//     14 independent 16-byte loads per lane), for h >= kPrevLoads one segment and its rows in groups of kPrevLoads ANDed into a running
//     value.  INVARIANT (the kernel's register budget, the fold planner's): at most kPrevMaxLoads = 16 loads of 4 VGPRs each per lane
//     and step; the kernel's arrays are sized by it and tests/test_kmer_prevalence_host.py checks it for every plan.
//   - Workgroups: as many wavefronts as the index has segments, at most kBlock / 64 (narrow indexes: as plan_col_popcount).  The
//     wavefronts of a workgroup are consecutive slices of the same slot, then the next slot.  grid <= 2 x kPrevWaves.
//   - The partial array: partial[slice][slot], slices x partial_stride entries (of one uint32, or two with a subset).
constexpr int kPrevLoads = 8;
constexpr int kPrevMaxLoads = 16;
constexpr uint64_t kPrevWaves = kColPopWaves;
struct PrevalencePlan {
    uint32_t block = 64;             // threads per workgroup
    uint32_t segs = 1;               // 1 KiB column segments that carry columns (at least 1)
    uint32_t slices = 1;             // per k-mer
    uint32_t segs_per_slice = 1;
    uint64_t waves_per_slice = 0;    // wavefronts that stride over the slots of one slice
    uint64_t waves = 0;              // slices x waves_per_slice
    uint64_t grid = 0;               // workgroups (0: nothing to sweep)
    uint32_t segs_per_step = 1;      // segments a lane takes at once
    uint32_t loads_per_step = 1;     // independent 16-byte loads a lane has in flight in a step
    uint64_t partial_stride = 0;     // entries per slice: one per slot
    uint64_t partial_entries = 0;    // slices x partial_stride
};
static inline uint32_t prevalence_segs_per_step(uint32_t h)
{
    return h >= (uint32_t)kPrevLoads ? 1u : (uint32_t)ceil_div(kPrevLoads, std::max<uint32_t>(h, 1));
}
// `wv`: 64-column words that carry columns; `total_pos` slots, `total_unique` of them unique k-mers
static inline PrevalencePlan plan_kmer_prevalence(uint64_t total_pos, uint64_t total_unique, uint64_t wv, uint32_t h)
{
    PrevalencePlan p;
    p.segs = (uint32_t)std::max<uint64_t>(ceil_div(wv, 64 * kVec), 1);
    p.block = (uint32_t)std::min<uint64_t>(p.segs, kBlock / 64) * 64;
    const uint64_t want_slices = std::min<uint64_t>(ceil_div(kPrevWaves, std::max<uint64_t>(total_unique, 1)), p.segs);
    p.segs_per_slice = (uint32_t)ceil_div(p.segs, want_slices);
    p.slices = (uint32_t)ceil_div(p.segs, p.segs_per_slice);
    p.waves_per_slice = std::min<uint64_t>(total_pos, std::max<uint64_t>(kPrevWaves / p.slices, 1));
    if (total_pos <= 2 * p.waves_per_slice) p.waves_per_slice = total_pos;
    p.waves = p.waves_per_slice * p.slices;
    p.grid = ceil_div(p.waves, p.block / 64);
    p.segs_per_step = prevalence_segs_per_step(h);
    p.loads_per_step = std::min<uint32_t>(std::max<uint32_t>(h, 1), kPrevLoads) * std::min<uint32_t>(p.segs_per_step, p.segs_per_slice);
    p.partial_stride = total_pos;
    p.partial_entries = p.slices * p.partial_stride;
    return p;
}

// ------------------------------------------------------------------------------ column collapse (k_collapse_columns)
// "OR these columns together": group_of[c] names the destination column of source column c (kCollapseDropped: none), and destination
// column g of every row is the OR of the source columns of group g.  The map is the same for all rows, so everything that depends on
// it alone is worked out HERE, once per call -- the row format's bit permutation included, so the kernel never maps a word to column
// order and back.  The tables speak of bits AS THEY LIE IN MEMORY: bit b of the little-endian 64-bit word w of a row is column
// 64 w + 8 (b / 8) + 7 - b % 8 (collapse_mem_bit is that permutation, and its own inverse).
//   - dst_bit[64 w + b]: the destination bit address 64 w' + b' of source bit (w, b), or kCollapseDropped.  4 bytes per source column
//     (400 KB at 100 k columns: resident in every XCD's L2).  The kernel reads it 32 bits at a time -- bit address a lies in the
//     little-endian 32-bit word a / 32 at bit a % 32 --, for the source's loads and for the LDS image's ORs alike.
//   - live[w]: the bits of source word w that have a destination.  The kernel ANDs a loaded word with it first, so dropped columns
//     and stray bits behind num_cols cost nothing and dst_bit is consulted only for bits that move.  live is what decides: a dst_bit
//     entry is never compared with kCollapseDropped on the device (the bit address of column 2^32 - 8 IS that value).
//     Both tables are padded to an even number of source words (the kernel's 16-byte loads; the padding is zero / dropped).
// Launch shape: a wavefront owns whole rows, one at a time, and an image of the destination row in LDS; about kCollapseWaves
// wavefronts stride over the rows.  The figure is INHERITED from the column popcounts' sweep (kColPopWaves, measured there), not
// measured for this kernel.  A handful of rows gets fewer wavefronts per workgroup.
// Window: the image is bounded by kCollapseWindowWords 64-bit words per wavefront (2048 = 16 KiB = 131 072 groups: the 100 k-sample
// index takes one pass; 4 wavefronts x 16 KiB = 64 KiB per workgroup, two workgroups per CU.  UNMEASURED starting values).  A wider
// destination is done in ceil(dst_words / window) windows per row: each pass over the source row keeps the bits whose destination lies
// in the window [win0, win0 + window) and the row comes from L2 after the first pass.  A narrow destination takes a smaller image
// (more workgroups per CU).  INVARIANTS (tests/test_collapse_columns_host.py checks them over seeded shapes): image_words is even and
// <= window_words; lds_bytes = image_words x 8 x wavefronts per workgroup <= kCollapseLdsBytes; the windows tile [0, dst_words)
// without gap or overlap.
constexpr uint32_t kCollapseDropped = 0xFFFFFFFFu;
constexpr uint64_t kCollapseWaves = kColPopWaves;
constexpr uint64_t kCollapseWindowWords = 2048;
constexpr uint64_t kCollapseLdsBytes = 64 * 1024;
constexpr int kCollapseLoads = 4;            // independent 16-byte loads a lane has in flight
constexpr int kCollapseGathers = 8;          // dst_bit gathers issued together, then that many LDS ORs
static_assert(kCollapseWindowWords % 2 == 0 && kCollapseWindowWords * 8 * (kBlock / 64) <= kCollapseLdsBytes, "the images of a workgroup fit its LDS");
static inline uint32_t collapse_mem_bit(uint32_t c) { return ((c >> 3) & 7u) * 8u + 7u - (c & 7u); }
struct CollapsePlan {
    uint64_t src_words = 0;          // ceil(num_cols / 64)
    uint64_t table_words = 0;        // src_words rounded up to even: live has that many entries, dst_bit 64 times as many
    uint64_t dst_words = 0;          // ceil(num_groups / 64)
    uint64_t window_words = 0;       // destination words per window
    uint64_t windows = 1;            // passes per row (at least 1)
    uint64_t image_words = 0;        // 64-bit words of one wavefront's LDS image
    uint32_t block = 64;             // threads per workgroup
    uint64_t grid = 0;               // workgroups; the wavefronts stride over the rows
    uint64_t lds_bytes = 0;          // dynamic LDS per workgroup
    uint64_t moved = 0;              // source columns that have a destination
    std::vector<uint32_t> dst_bit;   // 64 x table_words
    std::vector<uint64_t> live;      // table_words
};
// the first column whose entry is neither a group id nor kCollapseDropped, or num_cols
static inline uint64_t collapse_first_bad(uint64_t num_cols, const uint32_t *group_of, uint64_t num_groups)
{
    for (uint64_t c = 0; c < num_cols; c++)
        if (group_of[c] != kCollapseDropped && group_of[c] >= num_groups) return c;
    return num_cols;
}
// window j of a plan: destination words [first, first + count)
static inline void collapse_window(const CollapsePlan &p, uint64_t j, uint64_t *first, uint64_t *count)
{
    *first = j * p.window_words;
    *count = std::min<uint64_t>(p.window_words, p.dst_words - std::min(p.dst_words, *first));
}
// `group_of`: num_cols entries, each < num_groups or kCollapseDropped (collapse_first_bad); 0 < num_groups < 2^32 - 1
static inline CollapsePlan plan_collapse_columns(uint64_t num_cols, const uint32_t *group_of, uint64_t num_groups, uint64_t num_rows,
                                                 uint64_t window_words = kCollapseWindowWords)
{
    CollapsePlan p;
    p.src_words = ceil_div(num_cols, 64);
    p.table_words = round_up(p.src_words, 2);
    p.dst_words = ceil_div(num_groups, 64);
    p.window_words = window_words;
    p.windows = std::max<uint64_t>(ceil_div(p.dst_words, p.window_words), 1);
    p.image_words = std::min<uint64_t>(p.window_words, round_up(std::max<uint64_t>(p.dst_words, 1), 2));
    p.dst_bit.assign(p.table_words * 64, kCollapseDropped);
    p.live.assign(p.table_words, 0ull);
    for (uint64_t c = 0; c < num_cols; c++) {
        const uint32_t g = group_of[c];
        if (g == kCollapseDropped) continue;
        const uint32_t b = collapse_mem_bit((uint32_t)(c & 63));
        p.dst_bit[(c & ~63ull) + b] = (g & ~63u) + collapse_mem_bit(g & 63u);
        p.live[c >> 6] |= 1ull << b;
        p.moved++;
    }
    const uint64_t rows = std::max<uint64_t>(num_rows, 1);
    const uint64_t waves_per_block = std::min<uint64_t>(rows, kBlock / 64);
    p.block = (uint32_t)waves_per_block * 64;
    p.grid = std::min<uint64_t>(ceil_div(rows, waves_per_block), kCollapseWaves / (kBlock / 64));
    p.lds_bytes = p.image_words * 8 * waves_per_block;
    return p;
}

// ------------------------------------------------------------------------------ consensus collapse (k_consensus_columns<FIELD_BITS>)
// "Keep a bit where at least need[g] members have it": the collapse's map (group_of, kCollapseDropped), and destination column g of a
// row is 1 iff at least min_members[g] source columns of group g are set in it.  The LDS image of a wavefront holds COUNTERS instead
// of bits: one field of field_bits bits per group, 32 / field_bits of them packed into a 32-bit word (group c of a window that starts
// at group lo is field (c - lo) % per_word of word (c - lo) / per_word).
//   - live[w]: as the collapse's.
//   - dst_col[a]: the destination COLUMN NUMBER of source bit address a (bits as they lie in memory: collapse_mem_bit on the source
//     side only), or kCollapseDropped; as dst_bit, never compared with the sentinel on the device.
//   - sizes[g]: the members of group g.  field_bits = the smallest of 8, 16, 32 whose maximum (255, 65 535, 2^32 - 1) is at least
//     the largest size.  INVARIANT: a field's count never exceeds its group's size (a source column is added once per row) and the
//     size never exceeds the field maximum, so no add ever carries into a neighbouring field.
//   - need[64 w + l] = min_members[64 w + collapse_mem_bit(l)] for the destination word w: the order in which the lanes of the
//     read-out hold the word's bits, so lane l loads entry 64 w + l (coalesced) and the ballot of count >= need IS the memory word.
//     Padded with kConsensusNever up to round_up(dst_words, 2) words -- everything the read-out touches --, so the kernel never tests
//     a group bound: a count is at most 2^32 - 2 (fewer than 2^32 - 1 columns) and never reaches it.
// Window: a wavefront's image is at most kCollapseWindowWords x 8 bytes, as the collapse's, so a window holds
// kCollapseWindowWords / field_bits destination words = 16 384, 8192 or 4096 groups (1000 groups of at most 255 members: one window).
// image_words counts 64-bit LDS words like the collapse's: destination words of the image x field_bits.  Launch shape as
// plan_collapse_columns: kCollapseWaves is INHERITED there from the column popcounts' sweep and inherited again here, measured for
// neither kernel; kCollapseWindowWords is the collapse's UNMEASURED starting value.  INVARIANTS
// (tests/test_consensus_columns_host.py): window_words is even; image_words is a multiple of 2 x field_bits and
// <= kCollapseWindowWords at the planner's window; lds_bytes = image_words x 8 x wavefronts per workgroup <= kCollapseLdsBytes; the
// windows (collapse_window's rule) tile [0, dst_words) without gap or overlap.
constexpr uint32_t kConsensusNever = 0xFFFFFFFFu;
struct ConsensusPlan {
    uint64_t src_words = 0;          // ceil(num_cols / 64)
    uint64_t table_words = 0;        // src_words rounded up to even: live has that many entries, dst_col 64 times as many
    uint64_t dst_words = 0;          // ceil(num_groups / 64)
    uint32_t field_bits = 8;         // 8, 16 or 32
    uint64_t largest = 0;            // members of the largest group
    uint64_t window_words = 0;       // destination words per window (even)
    uint64_t windows = 1;            // passes per row (at least 1)
    uint64_t image_words = 0;        // 64-bit words of one wavefront's LDS image
    uint32_t block = 64;             // threads per workgroup
    uint64_t grid = 0;               // workgroups; the wavefronts stride over the rows
    uint64_t lds_bytes = 0;          // dynamic LDS per workgroup
    uint64_t moved = 0;              // source columns that have a destination
    std::vector<uint32_t> dst_col;   // 64 x table_words
    std::vector<uint64_t> live;      // table_words
    std::vector<uint32_t> sizes;     // num_groups
    std::vector<uint32_t> need;      // 64 x round_up(dst_words, 2)
};
static inline uint32_t consensus_field_bits(uint64_t largest) { return largest <= 0xFFull ? 8u : largest <= 0xFFFFull ? 16u : 32u; }
// the first group whose min_members entry is 0, or num_groups
static inline uint64_t consensus_first_zero(const uint32_t *min_members, uint64_t num_groups)
{
    for (uint64_t g = 0; g < num_groups; g++)
        if (min_members[g] == 0) return g;
    return num_groups;
}
// window j of a plan: destination words [first, first + count)
static inline void consensus_window(const ConsensusPlan &p, uint64_t j, uint64_t *first, uint64_t *count)
{
    *first = j * p.window_words;
    *count = std::min<uint64_t>(p.window_words, p.dst_words - std::min(p.dst_words, *first));
}
// `group_of` as for plan_collapse_columns; `min_members`: num_groups entries (NULL: the tables that need it stay empty);
// window_words 0: the planner's own, otherwise an even number of destination words
static inline ConsensusPlan plan_consensus_columns(uint64_t num_cols, const uint32_t *group_of, uint64_t num_groups, const uint32_t *min_members,
                                                   uint64_t num_rows, uint64_t window_words = 0)
{
    ConsensusPlan p;
    p.src_words = ceil_div(num_cols, 64);
    p.table_words = round_up(p.src_words, 2);
    p.dst_words = ceil_div(num_groups, 64);
    p.dst_col.assign(p.table_words * 64, kCollapseDropped);
    p.live.assign(p.table_words, 0ull);
    p.sizes.assign(num_groups, 0u);
    for (uint64_t c = 0; c < num_cols; c++) {
        const uint32_t g = group_of[c];
        if (g == kCollapseDropped) continue;
        const uint32_t b = collapse_mem_bit((uint32_t)(c & 63));
        p.dst_col[(c & ~63ull) + b] = g;
        p.live[c >> 6] |= 1ull << b;
        p.sizes[g]++;
        p.moved++;
    }
    for (uint32_t s : p.sizes) p.largest = std::max<uint64_t>(p.largest, s);
    p.field_bits = consensus_field_bits(p.largest);
    p.window_words = window_words ? window_words : kCollapseWindowWords / p.field_bits;
    p.windows = std::max<uint64_t>(ceil_div(p.dst_words, p.window_words), 1);
    p.image_words = std::min<uint64_t>(p.window_words, round_up(std::max<uint64_t>(p.dst_words, 1), 2)) * p.field_bits;
    if (min_members) {
        p.need.assign(round_up(p.dst_words, 2) * 64, kConsensusNever);
        for (uint64_t g = 0; g < num_groups; g++) p.need[(g & ~63ull) + collapse_mem_bit((uint32_t)(g & 63))] = min_members[g];
    }
    const uint64_t rows = std::max<uint64_t>(num_rows, 1);
    const uint64_t waves_per_block = std::min<uint64_t>(rows, kBlock / 64);
    p.block = (uint32_t)waves_per_block * 64;
    p.grid = std::min<uint64_t>(ceil_div(rows, waves_per_block), kCollapseWaves / (kBlock / 64));
    p.lds_bytes = p.image_words * 8 * waves_per_block;
    return p;
}

// ------------------------------------------------------------------------------ pairwise popcounts (k_columns_to_planes, k_pair_popcount, k_pair_popcount_sum)
// out[i][j] = |column cols_a[i] AND column cols_b[j]| over the rows: the bit-matrix product B^T B of the selected columns, the first
// compute-bound sweep here.  The rows are taken in CHUNKS; per chunk three launches on the index stream:
//   1. k_columns_to_planes transposes the distinct selected columns of the chunk into planes[u][chunk_words]: one 64-bit word per
//      column and 64-row group (a wavefront owns the group, a lane a row, a ballot makes the word).  Rows at or beyond num_rows come
//      out as 0, so what an in-place fold left behind num_rows is never counted.
//   2. k_pair_popcount: a workgroup owns a kPairTile x kPairTile tile of (distinct A column, distinct B column) pairs and one SLICE
//      of the chunk's words, stages both plane tiles kPairStageWords words at a time in LDS, every thread keeps a 4 x 4 block of
//      32-bit counters and writes them to partial[slice][ua][ub].  Symmetric calls (cols_b == NULL) run the tiles tj >= ti only.
//   3. k_pair_popcount_sum adds the slices of the chunk into the 64-bit [na][nb] device matrix (the first chunk assigns), through the
//      maps from list position to distinct column -- repeats are expanded here -- and, for symmetric calls, from the mirror tile.
// No global atomics, no workgroup waits for another.
// The host tables (PairwiseTables): the distinct columns of both lists in ascending order (= ascending source word, so a loaded word
// serves all of its selected columns and a 128-byte line is fetched once per 64-row group), as `words` (distinct source words),
// `first` (the planes of word k are first[k] .. first[k + 1]) and `bit` (the plane's bit in its word AS IT LIES IN MEMORY,
// collapse_mem_bit); plane_a / plane_b: the plane of the u-th distinct column of a list; map_a / map_b: list position -> u.
// The plan:
//   - chunk_words (64-row words per chunk): what kPairPlaneBytes of planes hold for the distinct columns (at most na_unique +
//     nb_unique of them; symmetric: na_unique), at least 2, at most kPairMaxChunkWords; and from kPairSplitWords words (2048 rows)
//     on never more than a third of the rows, so that every index of a few thousand rows already adds up three chunks (six more
//     launches on a large index that would have fitted one).
//   - slices: enough that tiles x slices reaches kPairWantGroups workgroups (8 per CU: the LDS of a workgroup is 32.5 KiB, four
//     fit a CU), at least two, no slice below kPairMinSliceWords words unless that leaves one slice, and no more than
//     kPairPartialBytes of partials hold (a selection of more than 2^27 distinct pairs has ONE slice: its partials alone are
//     over 512 MiB).  The last slice and the last chunk are ragged; no slice is empty.
//   - overflow: a 32-bit counter sees at most 64 x slice_words <= 64 x kPairMaxChunkWords = 2^30 rows.
// Scratch (PairwisePlan::plane_bytes + partial_bytes, independent of num_rows): plane_bytes <= max(kPairPlaneBytes, 16 x distinct
// columns), partial_bytes <= max(kPairPartialBytes, 4 x na_unique x nb_unique) -- 1.5 GiB for anything up to 2^26 distinct columns
// and 2^28 distinct pairs; the tables are 12 bytes per distinct column and 4 per list entry beside it.
// UNMEASURED starting values: kPairTile, the 4 x 4 register block, kPairStageWords, kPairWantGroups, kPlaneLoads.
constexpr uint64_t kPairwiseMaxPairs = 1ull << 28;          // na x nb of one call (2 GiB of uint64): BIGSI_PAIRWISE_MAX_PAIRS
constexpr int kPairTile = 64;                                // distinct columns per tile side
constexpr int kPairReg = 4;                                  // a thread's block is kPairReg x kPairReg pairs (16 x 16 threads)
constexpr int kPairStageWords = 32;                          // 64-row words of both tiles staged in LDS at a time
constexpr int kPairLdsStride = kPairTile + 2;                // 64-bit words per staged word (the pad spreads the staging stores over the banks; even: 16-byte reads)
constexpr int kPlaneLoads = 4;                               // independent 8-byte row loads a lane has in flight in k_columns_to_planes
constexpr uint64_t kPairPlaneBytes = 512ull << 20;
constexpr uint64_t kPairPartialBytes = 1ull << 30;
constexpr uint64_t kPairMaxChunkWords = 1ull << 24;
constexpr uint64_t kPairSplitWords = 32;
constexpr uint64_t kPairSplitChunks = 3;
constexpr uint64_t kPairMinSliceWords = 4;
constexpr uint64_t kPairWantGroups = 2048;
static_assert(kPairTile == 16 * kPairReg && kBlock == 16 * 16, "16 x 16 threads of kPairReg x kPairReg pairs cover a tile");
static_assert(kBlock % kPairStageWords == 0 && kPairTile % (kBlock / kPairStageWords) == 0, "the staging loop covers a tile in whole passes");
struct PairwisePlan {
    uint64_t total_words = 0;        // ceil(num_rows / 64)
    uint64_t chunk_words = 0;        // words per chunk = the stride of a plane
    uint64_t chunks = 0;
    uint64_t slice_words = 0;        // words per slice
    uint64_t slices = 0;             // of a full chunk
    uint64_t tiles_i = 0, tiles_j = 0;
    uint64_t tiles = 0;              // workgroups per slice: tiles_i x tiles_j (symmetric: those below the diagonal leave at once)
    uint64_t plane_bytes = 0, partial_bytes = 0;
};
// words of chunk c / slices of a chunk of `words` words
static inline uint64_t pairwise_chunk_words(const PairwisePlan &p, uint64_t c) { return std::min(p.chunk_words, p.total_words - std::min(p.total_words, c * p.chunk_words)); }
static inline uint64_t pairwise_chunk_slices(const PairwisePlan &p, uint64_t words) { return ceil_div(words, p.slice_words); }
// na_unique, nb_unique >= 1 distinct columns (symmetric: nb_unique == na_unique); num_rows >= 1; `stride_words` bounds the distinct columns
static inline PairwisePlan plan_pairwise(uint64_t na_unique, uint64_t nb_unique, bool symmetric, uint64_t num_rows, uint64_t stride_words)
{
    PairwisePlan p;
    const uint64_t distinct = std::min<uint64_t>(symmetric ? na_unique : na_unique + nb_unique, std::max<uint64_t>(stride_words, 1) * 64);
    p.total_words = std::max<uint64_t>(ceil_div(num_rows, 64), 1);
    const uint64_t budget_words = std::min(std::max<uint64_t>(kPairPlaneBytes / (8 * distinct), 2), kPairMaxChunkWords);
    p.chunk_words = std::min(budget_words, p.total_words >= kPairSplitWords ? ceil_div(p.total_words, kPairSplitChunks) : p.total_words);
    p.chunks = ceil_div(p.total_words, p.chunk_words);
    p.tiles_i = ceil_div(na_unique, kPairTile);
    p.tiles_j = ceil_div(nb_unique, kPairTile);
    p.tiles = p.tiles_i * p.tiles_j;
    const uint64_t active = symmetric ? p.tiles_i * (p.tiles_i + 1) / 2 : p.tiles;
    const uint64_t per_slice = 4 * na_unique * nb_unique;
    const uint64_t by_budget = std::max<uint64_t>(kPairPartialBytes / per_slice, 1);
    const uint64_t want = std::min(std::min(std::max<uint64_t>(ceil_div(kPairWantGroups, active), 2), by_budget), p.chunk_words);
    p.slice_words = std::max(ceil_div(p.chunk_words, want), std::min(kPairMinSliceWords, by_budget > 1 ? ceil_div(p.chunk_words, 2) : p.chunk_words));
    p.slices = ceil_div(p.chunk_words, p.slice_words);
    p.plane_bytes = distinct * p.chunk_words * 8;
    p.partial_bytes = p.slices * per_slice;
    return p;
}

struct PairwiseTables {
    std::vector<uint32_t> words, first, bit;          // first has words.size() + 1 entries, bit one per plane
    std::vector<uint32_t> plane_a, plane_b;           // distinct column of a list -> plane (symmetric: plane_b is empty)
    std::vector<uint32_t> map_a, map_b;               // list position -> distinct column of the list (symmetric: map_b is empty)
};
// the first entry of a list that is no column of the index, or n
static inline uint64_t pairwise_first_bad(const uint32_t *cols, uint64_t n, uint64_t num_cols)
{
    for (uint64_t i = 0; i < n; i++)
        if (cols[i] >= num_cols) return i;
    return n;
}
// cols_b == nullptr: symmetric
static inline PairwiseTables pairwise_tables(const uint32_t *cols_a, uint64_t na, const uint32_t *cols_b, uint64_t nb)
{
    PairwiseTables t;
    std::vector<uint32_t> ua(cols_a, cols_a + na), ub, all;
    std::sort(ua.begin(), ua.end());
    ua.erase(std::unique(ua.begin(), ua.end()), ua.end());
    if (cols_b) {
        ub.assign(cols_b, cols_b + nb);
        std::sort(ub.begin(), ub.end());
        ub.erase(std::unique(ub.begin(), ub.end()), ub.end());
        all.resize(ua.size() + ub.size());
        all.erase(std::set_union(ua.begin(), ua.end(), ub.begin(), ub.end(), all.begin()), all.end());
    } else
        all = ua;
    t.bit.reserve(all.size());
    for (uint32_t c : all) {
        if (t.words.empty() || t.words.back() != c >> 6) {
            t.words.push_back(c >> 6);
            t.first.push_back((uint32_t)t.bit.size());
        }
        t.bit.push_back(((c >> 3) & 7u) * 8u + 7u - (c & 7u));
    }
    t.first.push_back((uint32_t)t.bit.size());
    const auto rank = [](const std::vector<uint32_t> &in, uint32_t c) { return (uint32_t)(std::lower_bound(in.begin(), in.end(), c) - in.begin()); };
    t.plane_a.resize(ua.size());
    for (size_t u = 0; u < ua.size(); u++) t.plane_a[u] = rank(all, ua[u]);
    t.map_a.resize(na);
    for (uint64_t i = 0; i < na; i++) t.map_a[i] = rank(ua, cols_a[i]);
    if (cols_b) {
        t.plane_b.resize(ub.size());
        for (size_t u = 0; u < ub.size(); u++) t.plane_b[u] = rank(all, ub[u]);
        t.map_b.resize(nb);
        for (uint64_t j = 0; j < nb; j++) t.map_b[j] = rank(ub, cols_b[j]);
    }
    return t;
}

// ------------------------------------------------------------------------------ query-set tally (k_tally_hits, k_tally_totals)
// k_tally_hits: a wavefront owns ONE result word (64 columns, lane = column) and a tile of kTallyTile queries; the kBlock / 64
// wavefronts of a workgroup own neighbouring words of the same tile.  Workgroup b: word group b % word_groups, tile b / word_groups
// (neighbouring workgroups read neighbouring words of the same queries).  A tile costs every column of a hit word one pair of 64-bit
// atomics, so it is as long as keeps those rare (at most ceil(n_seqs / 128) pairs per column and batch) and as short as still gives a
// narrow index some workgroups.  k_tally_totals: a workgroup owns kTallyTotalsTile queries, a wavefront every fourth of them -- one each:
// a wavefront sweeps a query's words one load latency after the other, and 8192 queries of 1563 words on 64-query workgroups were 512
// wavefronts on a device that holds 8192 (measured, both kernels per 8192 queries: 1.55 ms at 64, 0.63 ms at 4).
constexpr uint32_t kTallyTile = 128;
constexpr uint32_t kTallyLoads = 8;               // result words a wavefront has in flight
constexpr uint32_t kTallyTotalsTile = 4;
struct TallyPlan {
    uint32_t block = kBlock, tile = kTallyTile;
    uint64_t word_groups = 0, tiles = 0, grid = 0;            // grid = word_groups * tiles
    uint64_t totals_grid = 0;
    uint64_t too_large = 0;                                   // != 0: the workgroups one launch would take (more than 2^31 - 1): refused
};
static inline TallyPlan plan_tally(uint64_t n_seqs, uint64_t wv)
{
    TallyPlan p;
    p.word_groups = ceil_div(wv, kBlock / 64);
    p.tiles = ceil_div(n_seqs, p.tile);
    p.grid = p.word_groups * p.tiles;
    p.totals_grid = ceil_div(n_seqs, kTallyTotalsTile);
    if (p.tiles && p.word_groups > 0x7FFFFFFFull / p.tiles) p.too_large = p.word_groups * p.tiles;
    return p;
}

// The device batches of bigsi_hip_tally_add_stream: sequences [cut[i], cut[i + 1]) of the input, greedily as long as a chunk holds at
// most kTallyChunkSeqs sequences, kTallyChunkPositions k-mer positions and kTallyCounterBytes of dense counters
// (n_seqs * wv_pad * 64 * count_bytes: what a counting run allocates; count_bytes 0 for an exact stream, which has none) -- and always
// at least one sequence, so that a single sequence beyond a bound is a chunk of its own.  The planner takes the counter width it is
// given: the stream passes 4, the wider of the two a run may pick, so the bound holds whichever it picks.
constexpr uint64_t kTallyChunkSeqs = 4096;
constexpr uint64_t kTallyChunkPositions = 1ull << 20;
constexpr uint64_t kTallyCounterBytes = 2ull << 30;          // BIGSI_TALLY_COUNTER_BYTES (include/bigsi_hip_tally.h)
// end of the chunk that starts at sequence s0 < n_seqs
static inline uint64_t tally_chunk_end(const uint64_t *offsets, uint64_t n_seqs, uint64_t s0, uint32_t k, uint64_t wv_pad, uint32_t count_bytes)
{
    const uint64_t per_seq = wv_pad * 64 * count_bytes;
    const uint64_t by_bytes = per_seq ? std::max<uint64_t>(kTallyCounterBytes / per_seq, 1) : kTallyChunkSeqs;
    const uint64_t most = std::min(std::min(kTallyChunkSeqs, by_bytes), n_seqs - s0);
    uint64_t pos = 0, s = s0;
    while (s < s0 + most) {
        const uint64_t len = offsets[s + 1] - offsets[s], n = len >= k ? len - k + 1 : 0;
        if (s > s0 && pos + n > kTallyChunkPositions) break;
        pos += n;
        s++;
    }
    return s;
}
static inline std::vector<uint64_t> plan_tally_chunks(const uint64_t *offsets, uint64_t n_seqs, uint32_t k, uint64_t wv_pad, uint32_t count_bytes)
{
    std::vector<uint64_t> cut(1, 0);
    while (cut.back() < n_seqs) cut.push_back(tally_chunk_end(offsets, n_seqs, cut.back(), k, wv_pad, count_bytes));
    return cut;
}

// ------------------------------------------------------------------------------ read classification (k_classify_groups)
// One workgroup of kBlock threads per query.  Dynamic LDS: the per-group table best[n_groups] (uint64) | hits[n_groups] (uint32), rounded
// up to 16 bytes, and behind it three uint64 per wavefront for the final reduction -- 48 KiB + 96 bytes at kClassifyMaxGroups, three
// workgroups per CU; a table of a hundred groups does not bound the occupancy.  A query whose result vector is empty leaves before it
// touches the table (pass 1 of the kernel), so the grid is the batch, whatever the hit density.  Refused: more than 2^31 - 1 workgroups,
// n_groups outside 1 .. kClassifyMaxGroups.
constexpr uint32_t kClassifyMaxGroups = 4096;               // BIGSI_CLASSIFY_MAX_GROUPS (include/bigsi_hip_classify.h)
constexpr uint32_t kClassifyNoGroup = 0xFFFFFFFFu;          // BIGSI_CLASSIFY_NONE
struct ClassifyPlan {
    uint32_t block = kBlock;
    uint64_t grid = 0;
    uint32_t table_bytes = 0, lds_bytes = 0;                  // the table alone; with the wavefronts' partial results (the launch's dynamic LDS)
    uint64_t too_large = 0;                                   // != 0: the workgroups one launch would take (more than 2^31 - 1): refused
    bool bad_groups = false;                                  // n_groups is 0 or above kClassifyMaxGroups: refused
};
static inline ClassifyPlan plan_classify(uint64_t n_seqs, uint64_t wv, uint64_t n_groups)
{
    ClassifyPlan p;
    (void)wv;                                                 // (a workgroup sweeps its query's words itself: the width changes no launch figure)
    p.grid = n_seqs;
    if (n_seqs > 0x7FFFFFFFull) p.too_large = n_seqs;
    if (n_groups == 0 || n_groups > kClassifyMaxGroups) { p.bad_groups = true; return p; }
    p.table_bytes = (uint32_t)round_up(n_groups * 12, 16);
    p.lds_bytes = p.table_bytes + (kBlock / 64) * 3 * 8;
    return p;
}
// the first column whose group_of entry is neither below n_groups nor kClassifyNoGroup; n_entries when every entry is fine
static inline uint64_t classify_bad_column(const uint32_t *group_of, uint64_t n_entries, uint64_t n_groups)
{
    for (uint64_t c = 0; c < n_entries; c++)
        if (group_of[c] != kClassifyNoGroup && group_of[c] >= n_groups) return c;
    return n_entries;
}

// ------------------------------------------------------------------------------ group association (k_group_masks, k_group_counts)
// k_group_masks: one wavefront per result word, kBlock / 64 words per workgroup -> masks[n_groups][wv].  k_group_counts: a workgroup of
// kBlock threads takes kAssociateQueries queries and sweeps their wv words once per pass of kAssociateGroupBlock groups (GB), whose
// kAssociateQueries x GB partial counts stay in registers; static LDS holds the wavefronts' partial sums (the counts and, in the first
// pass, one samples_hit per query).  Refused: more than 2^31 - 1 workgroups in either launch, n_groups outside 1 .. kAssociateMaxGroups.
constexpr uint32_t kAssociateMaxGroups = 64;                // BIGSI_ASSOCIATE_MAX_GROUPS (include/bigsi_hip_associate.h)
constexpr uint32_t kAssociateNoGroup = 0xFFFFFFFFu;         // BIGSI_ASSOCIATE_NONE
static_assert(kAssociateNoGroup == kClassifyNoGroup, "classify_bad_column serves both");
constexpr uint32_t kAssociateQueries = 4;                   // queries per workgroup of k_group_counts
constexpr uint32_t kAssociateGroupBlock = 8;                // GB: groups per pass of k_group_counts
struct AssociatePlan {
    uint32_t block = kBlock;
    uint64_t grid = 0, mask_grid = 0;                         // k_group_counts; k_group_masks
    uint32_t lds_bytes = 0, passes = 0;                       // static LDS of k_group_counts; its passes over a query's result vector
    uint64_t mask_bytes = 0;                                  // masks[n_groups][wv]
    uint64_t too_large = 0;                                   // != 0: the workgroups one launch would take (more than 2^31 - 1): refused
    bool bad_groups = false;                                  // n_groups is 0 or above kAssociateMaxGroups: refused
};
static inline AssociatePlan plan_associate(uint64_t n_seqs, uint64_t wv, uint64_t n_groups)
{
    AssociatePlan p;
    p.grid = (n_seqs + kAssociateQueries - 1) / kAssociateQueries;
    p.mask_grid = (wv + kBlock / 64 - 1) / (kBlock / 64);
    p.lds_bytes = (kBlock / 64) * kAssociateQueries * (kAssociateGroupBlock + 1) * 4;
    if (p.grid > 0x7FFFFFFFull) p.too_large = p.grid;
    else if (p.mask_grid > 0x7FFFFFFFull) p.too_large = p.mask_grid;
    if (n_groups == 0 || n_groups > kAssociateMaxGroups) { p.bad_groups = true; return p; }
    p.passes = (uint32_t)((n_groups + kAssociateGroupBlock - 1) / kAssociateGroupBlock);
    p.mask_bytes = n_groups * wv * 8;
    return p;
}

// ------------------------------------------------------------------------------ panel genotyping (k_allele_or, k_genotype_variants, k_genotype_samples)
// k_allele_or: thread = result word, a workgroup owns kBlock consecutive words and one tile of kGenotypeTile probes; workgroup b: word
// block b % word_blocks, tile b / word_blocks (the tally's order: neighbouring workgroups read neighbouring words of the same probes).
// A tile costs a word one 64-bit atomic per allele it holds, so it is as long as keeps those rare and as short as still gives a narrow
// index some workgroups; it is at most kBlock, since thread i of the workgroup that owns word 0 counts probe i of the tile into `used`.
// k_genotype_variants: one wavefront per variant, kBlock / 64 per workgroup.  k_genotype_samples: one wavefront per result word.
// plane_bytes is both planes of all variants as the device holds them (rows of wv words).  Refused: n_variants outside 1 ..
// kGenotypeMaxVariants, planes above kGenotypePlaneBytes, more than 2^31 - 1 workgroups in a launch.
constexpr uint32_t kGenotypeNone = 0xFFFFFFFFu;             // BIGSI_GENOTYPE_NONE (include/bigsi_hip_genotype.h)
constexpr uint32_t kGenotypeMaxVariants = 1u << 20;         // BIGSI_GENOTYPE_MAX_VARIANTS
constexpr uint64_t kGenotypePlaneBytes = 4ull << 30;        // BIGSI_GENOTYPE_PLANE_BYTES: a design limit, not a measured one
constexpr uint32_t kGenotypeTile = 64;                      // probes per workgroup of k_allele_or
constexpr uint32_t kGenotypeLoads = 8;                      // result words a thread of k_allele_or has in flight
static_assert(kGenotypeTile <= (uint32_t)kBlock && kGenotypeTile % kGenotypeLoads == 0, "k_allele_or: thread i counts probe i; whole load groups");
struct GenotypePlan {
    uint32_t block = kBlock, tile = kGenotypeTile;
    uint64_t word_blocks = 0, tiles = 0, grid = 0;            // k_allele_or: grid = word_blocks * tiles
    uint64_t variants_grid = 0, samples_grid = 0;             // k_genotype_variants; k_genotype_samples
    uint64_t plane_bytes = 0;                                 // planes[2 n_variants][wv]
    uint64_t too_large = 0;                                   // != 0: the workgroups one launch would take (more than 2^31 - 1): refused
    bool bad_variants = false, too_many_bytes = false;        // n_variants outside 1 .. kGenotypeMaxVariants; planes above kGenotypePlaneBytes
};
static inline GenotypePlan plan_genotype(uint64_t n_seqs, uint64_t wv, uint64_t n_variants)
{
    GenotypePlan p;
    p.word_blocks = ceil_div(wv, (uint64_t)kBlock);
    p.tiles = ceil_div(n_seqs, (uint64_t)p.tile);
    p.grid = p.tiles && p.word_blocks > ~0ull / p.tiles ? ~0ull : p.word_blocks * p.tiles;      // (saturates: the product may not fit 64 bits)
    p.samples_grid = ceil_div(wv, (uint64_t)(kBlock / 64));
    if (p.grid > 0x7FFFFFFFull) p.too_large = p.grid;
    else if (p.samples_grid > 0x7FFFFFFFull) p.too_large = p.samples_grid;
    if (n_variants == 0 || n_variants > kGenotypeMaxVariants) { p.bad_variants = true; return p; }
    p.variants_grid = ceil_div(n_variants, (uint64_t)(kBlock / 64));
    if (wv > kGenotypePlaneBytes / (16 * n_variants)) p.too_many_bytes = true;      // (by division: the product may not fit 64 bits)
    else p.plane_bytes = 2 * n_variants * wv * 8;
    return p;
}
// the first allele_of entry that is neither below 2 n_variants nor kGenotypeNone; n_entries when there is none
static inline uint64_t genotype_bad_allele(const uint32_t *allele_of, uint64_t n_entries, uint64_t n_variants)
{
    for (uint64_t i = 0; i < n_entries; i++)
        if (allele_of[i] != kGenotypeNone && allele_of[i] >= 2 * n_variants) return i;
    return n_entries;
}

// ------------------------------------------------------------------------------ locus typing (k_locus_best, k_locus_counts)
// k_locus_best: the tally's shape -- a wavefront owns ONE result word (64 columns, lane = column) and a tile of kTypingTile records;
// the kBlock / 64 wavefronts of a workgroup own neighbouring words of the same tile; workgroup b: word group b % word_groups, tile
// b / word_groups.  A tile costs a column one 64-bit atomicMax and one 32-bit atomicAdd per locus it holds a hit of, so it is as long as
// keeps those rare and as short as still gives a narrow index some workgroups; it is at most kBlock, since thread i of the workgroup
// that owns word 0 counts record i of the tile into `records`.  k_locus_counts: one launch, two parts -- the first loci_grid
// workgroups give a wavefront to each locus, the words_grid behind them a wavefront to each result word.  cell_bytes is best (8 bytes)
// and hits (4 bytes) of every (locus, column) as the device holds them (rows of wv * 64 cells).  Refused: n_loci outside 1 ..
// kTypingMaxLoci, cells above kTypingCellBytes, more than 2^31 - 1 workgroups in a launch.
constexpr uint32_t kTypingNone = 0xFFFFFFFFu;               // BIGSI_TYPING_NONE (include/bigsi_hip_typing.h)
constexpr uint32_t kTypingMaxAllele = 0xFFFFFFFEu;          // BIGSI_TYPING_MAX_ALLELE
constexpr uint32_t kTypingMaxLoci = 1u << 20;               // BIGSI_TYPING_MAX_LOCI
constexpr uint64_t kTypingCellBytes = 4ull << 30;           // BIGSI_TYPING_CELL_BYTES: a design limit, not a measured one
constexpr uint32_t kTypingTile = 64;                        // records per workgroup of k_locus_best
constexpr uint32_t kTypingLoads = 8;                        // result words a wavefront of k_locus_best has in flight
static_assert(kTypingTile <= (uint32_t)kBlock && kTypingTile % kTypingLoads == 0, "k_locus_best: thread i counts record i; whole load groups");
// The key of a hit (include/bigsi_hip_typing.h): the fraction c / u of the record's k-mers found, as floor(c (2^32 - 1) / u), above the
// complement of the allele identity -- the highest fraction wins, ties go to the lowest identity, and the key of a hit is never 0.
// c <= u < 2^32 and u > 0: the product fits 64 bits.  Two different fractions share a score only when u_i * u_j > 2^32.  constexpr: the
// kernel and the host tests compile this one function, so its CPU pin is the pin of the kernel's arithmetic.
constexpr uint64_t typing_key(uint32_t c, uint32_t u, uint32_t allele)
{
    return ((uint64_t)c * 0xFFFFFFFFull / u) << 32 | (uint64_t)(0xFFFFFFFFu - allele);
}
struct TypingPlan {
    uint32_t block = kBlock, tile = kTypingTile;
    uint64_t word_groups = 0, tiles = 0, grid = 0;            // k_locus_best: grid = word_groups * tiles
    uint64_t loci_grid = 0, words_grid = 0, counts_grid = 0;  // k_locus_counts: counts_grid = loci_grid + words_grid
    uint64_t cell_bytes = 0;                                  // best[n_loci][wv * 64] (8 bytes) + hits[n_loci][wv * 64] (4 bytes)
    uint64_t too_large = 0;                                   // != 0: the workgroups one launch would take (more than 2^31 - 1): refused
    bool bad_loci = false, too_many_bytes = false;            // n_loci outside 1 .. kTypingMaxLoci; cells above kTypingCellBytes
};
static inline TypingPlan plan_typing(uint64_t n_seqs, uint64_t wv, uint64_t n_loci)
{
    TypingPlan p;
    p.word_groups = wv / (kBlock / 64) + (wv % (kBlock / 64) ? 1 : 0);      // (ceil without the sum: wv may be anything)
    p.tiles = ceil_div(n_seqs, (uint64_t)p.tile);
    p.grid = p.tiles && p.word_groups > ~0ull / p.tiles ? ~0ull : p.word_groups * p.tiles;      // (saturates: the product may not fit 64 bits)
    p.words_grid = p.word_groups;
    if (p.grid > 0x7FFFFFFFull) p.too_large = p.grid;
    if (n_loci == 0 || n_loci > kTypingMaxLoci) {
        p.bad_loci = true;
        if (!p.too_large && p.words_grid > 0x7FFFFFFFull) p.too_large = p.words_grid;
        return p;
    }
    p.loci_grid = ceil_div(n_loci, (uint64_t)(kBlock / 64));
    p.counts_grid = p.loci_grid + p.words_grid;               // (loci_grid <= 2^18 and words_grid <= 2^62: no overflow)
    if (!p.too_large && p.counts_grid > 0x7FFFFFFFull) p.too_large = p.counts_grid;
    if (wv > kTypingCellBytes / (768 * n_loci)) p.too_many_bytes = true;      // (by division: the product may not fit 64 bits)
    else p.cell_bytes = n_loci * wv * 768;
    return p;
}
// the first record whose labels are refused: a locus that is neither below n_loci nor kTypingNone, or -- for a record with a locus -- an
// allele identity above kTypingMaxAllele; n_entries when there is none.  The allele of a record without a locus is not looked at.
static inline uint64_t typing_bad_label(const uint32_t *locus_of, const uint32_t *allele_of, uint64_t n_entries, uint64_t n_loci)
{
    for (uint64_t i = 0; i < n_entries; i++)
        if (locus_of[i] != kTypingNone && (locus_of[i] >= n_loci || allele_of[i] > kTypingMaxAllele)) return i;
    return n_entries;
}

// ------------------------------------------------------------------------------ windowed search (k_window_max, k_window_combine)
// plan_window_search: sequence q of a batch has n[q] k-mer positions, a window of We = min(W, n[q]) of them and the window starts
// [0, n[q] - We]; the sweep cuts every sequence's starts into segments of at most S and a wavefront of k_window_max owns one
// (segment, tile of 64 x kVec column words).  A segment [a, b) costs We positions of warm-up plus 2 (b - a - 1) positions of steps.
//   - S: 4 x the largest We (at least 64) -- the warm-up is then a ninth of the traffic -- and shorter only while that leaves fewer
//     than kWindowWaves wavefronts, never below the largest We (at least 64: there the warm-up is a third).  kWindowWaves is INHERITED
//     from the column popcounts' sweep (kColPopWaves), not measured for this kernel.  `forced_starts` > 0 (bigsi_hip_window_set_limits)
//     is taken as it is.
//   - planes: the counters of a segment are `planes` bit planes, planes >= bit_width(largest We), in the buckets the kernel is
//     instantiated for (4, 8, 12, 16).
//   - partial: every (segment, plane) leaves wvp = round_up(wv, kVec) words: partial_bytes = n_segs x planes x wvp x 8, exactly.
//   - refusals: a grid above 2^31 - 1 workgroups (grid_too_large), partial_bytes above the cap (partial_too_large; cap 0 = 2 GiB, the
//     bound of the tally's dense counters).  The caller reports them with the numbers.
//   - steps_per_iter: window steps whose 2 h row loads a lane issues together: 4 / 2 / 1 for h = 1 / 2-3 / more -- 8 to 14 independent
//     16-byte loads in flight, as k_and_count keeps (h >= 8, the generic instantiation: one step, its rows one after the other).
constexpr uint64_t kWindowWaves = kColPopWaves;
constexpr uint64_t kWindowPartialBytes = 2ull << 30;
constexpr uint32_t kWindowMax = 65535;                       // BIGSI_WINDOW_MAX (include/bigsi_hip_window.h)
constexpr uint64_t kWindowMinSegment = 64;
struct WindowSeg {
    uint32_t q, a, b, we;      // window starts [a, b) of sequence q, whose window is `we` positions
};
struct WindowPlan {
    uint32_t max_we = 0;             // the largest window of the batch (0: no sequence has a position)
    uint32_t planes = 4;
    uint64_t seg_starts = 0;         // S
    uint32_t tiles = 1;              // wavefronts per segment: 64 x kVec words each
    uint64_t n_segs = 0, waves = 0, grid = 0;
    uint64_t wvp = 0;                // words per plane of a segment's entry
    uint64_t partial_bytes = 0;
    uint32_t steps_per_iter = 1;
    bool grid_too_large = false, partial_too_large = false;
    std::vector<WindowSeg> segs;
    std::vector<uint64_t> seg_off;   // n_seqs + 1: sequence q owns segs[seg_off[q], seg_off[q + 1])
};
static inline uint32_t window_bit_width(uint32_t x)
{
    uint32_t w = 0;
    while (x) { w++; x >>= 1; }
    return w;
}
static inline uint32_t window_plane_bucket(uint32_t we) { return std::max<uint32_t>((uint32_t)round_up(window_bit_width(we), 4), 4); }
static inline uint32_t window_steps_per_iter(uint32_t h) { return h <= 1 ? 4u : h <= 3 ? 2u : 1u; }
static inline WindowPlan plan_window_search(const uint32_t *n, uint32_t n_seqs, uint32_t window, uint64_t wv, uint32_t h,
                                            uint64_t forced_starts = 0, uint64_t partial_cap = 0)
{
    WindowPlan p;
    uint64_t starts = 0;
    for (uint32_t q = 0; q < n_seqs; q++) {
        const uint32_t we = std::min(n[q], window);
        if (!we) continue;
        p.max_we = std::max(p.max_we, we);
        starts += n[q] - we + 1;
    }
    p.planes = window_plane_bucket(p.max_we);
    p.tiles = (uint32_t)std::max<uint64_t>(ceil_div(wv, 64 * kVec), 1);
    p.wvp = round_up(wv, kVec);
    p.steps_per_iter = window_steps_per_iter(h);
    p.seg_off.assign((size_t)n_seqs + 1, 0);
    if (!p.max_we) return p;
    const uint64_t floor_s = std::max<uint64_t>(p.max_we, kWindowMinSegment), top_s = std::max<uint64_t>(4ull * p.max_we, kWindowMinSegment);
    if (forced_starts) p.seg_starts = forced_starts;
    else {
        const uint64_t want_segs = std::max<uint64_t>(ceil_div(kWindowWaves, p.tiles), 1);
        p.seg_starts = std::min(std::max(ceil_div(starts, want_segs), floor_s), top_s);
    }
    for (uint32_t q = 0; q < n_seqs; q++) {
        p.seg_off[q] = p.segs.size();
        const uint32_t we = std::min(n[q], window);
        if (!we) continue;
        const uint64_t nst = (uint64_t)n[q] - we + 1;
        for (uint64_t a = 0; a < nst; a += p.seg_starts) p.segs.push_back(WindowSeg{q, (uint32_t)a, (uint32_t)std::min(a + p.seg_starts, nst), we});
    }
    p.seg_off[n_seqs] = p.segs.size();
    p.n_segs = p.segs.size();
    p.waves = p.n_segs * p.tiles;
    p.grid = ceil_div(p.waves, kBlock / 64);
    p.partial_bytes = p.n_segs * p.planes * p.wvp * 8;
    p.grid_too_large = p.grid > 0x7FFFFFFFull;
    p.partial_too_large = p.partial_bytes > (partial_cap ? partial_cap : kWindowPartialBytes);
    return p;
}

// ------------------------------------------------------------------------------ exact k-mer counter (k_count_kmers, k_kmer_table_*)
// plan_kmer_count_add: everything bigsi_hip_kmer_counter_add decides from the offsets alone -- the call's positions, its refusal and the
// staging chunks -- BEFORE any byte behind `seqs` is touched (a refused call may name bytes it does not own: include/bigsi_cpu_kmercount.h).
// A chunk is a range [begin, end) of the call's bytes of at most `chunk_bytes`; the reads it meets are [seq0, seq1), the first and the
// last of them possibly in part.  Chunks are cut at read boundaries (the last boundary the limit allows); a read that reaches beyond
// begin + chunk_bytes is cut there and the next chunk begins k - 1 bytes earlier, so that every window lies whole in exactly one
// chunk.  The ranges run from offsets[0] to offsets[n_seqs] without a gap: each begins where the one before ended, or k - 1 before it.
// The device stages a chunk's pieces behind one another with one separator byte (no base) after every piece that is not empty.
constexpr uint64_t kKmerCountLifetime = 0xFFFFFFFFull;       // positions a counter takes in its lifetime (no uint32 count wraps)
constexpr uint64_t kKmerChunkBytes = 32ull << 20;            // staging chunk of bigsi_hip_kmer_counter_add (not measured: a few chunks per GB of reads)
constexpr uint64_t kKmerMinChunkBytes = 64;                  // >= 2 * BIGSI_KMERCOUNT_MAX_K: a cut read advances by chunk - (k - 1) > 0
constexpr uint64_t kKmerInitialSlots = 1ull << 16;
constexpr uint64_t kKmerMinSlots = 64;
constexpr uint32_t kKmerTile = 4096;                         // window starts of a workgroup of k_count_kmers: kKmerLane per thread
constexpr uint32_t kKmerLane = 16;                           // ... one 16-byte load and one 32-bit code word each
static_assert(kKmerTile == kBlock * kKmerLane, "a thread of k_count_kmers owns one code word of window starts");
struct KmerChunk {
    uint64_t begin = 0, end = 0;          // bytes [begin, end) behind seqs
    uint64_t seq0 = 0, seq1 = 0;          // the reads those bytes belong to
    uint64_t positions = 0;               // windows of the chunk's pieces
    uint64_t staged = 0;                  // bytes on the device: end - begin + one separator per non-empty piece
};
struct KmerAddPlan {
    enum Refusal { kNone = 0, kNotMonotone = 1, kLifetime = 2 } refusal = kNone;
    uint64_t bad_seq = 0;                 // kNotMonotone: the first read whose end lies before its start
    uint64_t positions = 0;               // of the whole call
    std::vector<KmerChunk> chunks;        // empty when refused
};
static inline uint64_t kmer_positions(uint64_t len, uint32_t k) { return len >= k ? len - k + 1 : 0; }
static inline KmerAddPlan plan_kmer_count_add(uint32_t k, const uint64_t *offsets, uint64_t n_seqs, uint64_t taken, uint64_t chunk_bytes)
{
    KmerAddPlan p;
    if (n_seqs == 0) return p;
    for (uint64_t i = 0; i < n_seqs; i++) {
        if (offsets[i + 1] < offsets[i]) { p.refusal = KmerAddPlan::kNotMonotone; p.bad_seq = i; p.positions = 0; return p; }
        p.positions += kmer_positions(offsets[i + 1] - offsets[i], k);          // (at most offsets[n_seqs] - offsets[0]: no overflow)
    }
    if (taken > kKmerCountLifetime || p.positions > kKmerCountLifetime - taken) { p.refusal = KmerAddPlan::kLifetime; return p; }
    chunk_bytes = std::max(chunk_bytes, kKmerMinChunkBytes);
    const uint64_t last = offsets[n_seqs];
    uint64_t cur = offsets[0], s = 0;          // read s holds byte cur (or starts there)
    while (cur < last) {
        KmerChunk c;
        c.begin = cur;
        while (offsets[s + 1] <= cur && s + 1 < n_seqs) s++;          // (empty reads at the cut, and the read a boundary cut ended)
        c.seq0 = s;
        const uint64_t reach = last - cur > chunk_bytes ? cur + chunk_bytes : last;
        const uint64_t j = (uint64_t)(std::upper_bound(offsets + s, offsets + n_seqs + 1, reach) - offsets) - 1;      // the last boundary <= reach
        uint64_t next;
        if (offsets[j] > cur) { c.end = offsets[j]; c.seq1 = j; next = c.end; }
        else { c.end = reach; c.seq1 = s + 1; next = reach - (k - 1); }          // inside read s, which reaches beyond `reach`
        for (uint64_t i = c.seq0; i < c.seq1; i++) {
            const uint64_t a = std::max(offsets[i], c.begin), b = std::min(offsets[i + 1], c.end);
            c.positions += kmer_positions(b - a, k);
            c.staged += b > a ? b - a + 1 : 0;
        }
        p.chunks.push_back(c);
        cur = next;
    }
    return p;
}

// A chunk's pieces behind one another in dst[0 .. c.staged), a separator byte (0: no base) behind every piece that is not empty, so
// that no window of the staged stream spans two pieces.  Reads seqs[c.begin .. c.end) and nothing else; returns the bytes written.
static inline uint64_t kmer_stage_chunk(const char *seqs, const uint64_t *offsets, const KmerChunk &c, uint8_t *dst)
{
    uint64_t at = 0;
    for (uint64_t i = c.seq0; i < c.seq1; i++) {
        const uint64_t a = std::max(offsets[i], c.begin), b = std::min(offsets[i + 1], c.end);
        if (b <= a) continue;
        std::copy(seqs + a, seqs + b, reinterpret_cast<char *>(dst) + at);
        at += b - a;
        dst[at++] = 0;
    }
    return at;
}

// The table rule: the slot count is a power of two, and before a chunk is launched distinct + positions_of_chunk <= slots / 2 holds
// -- every window of the chunk may be a new key, so k_count_kmers never meets a table more than half full and its probe sequences stay
// short; the host grows the table (k_kmer_table_rehash) to `slots` first when that is more than it has.  grid: the chunk's tiles.
struct KmerTablePlan {
    uint64_t slots = 0;
    bool grow = false;
    uint64_t grid = 0;
    uint32_t block = kBlock;
};
static inline KmerTablePlan plan_kmer_table(uint64_t slots_now, uint64_t distinct, uint64_t chunk_positions, uint64_t chunk_staged)
{
    KmerTablePlan p;
    p.slots = std::max(slots_now, kKmerMinSlots);
    while (p.slots & (p.slots - 1)) p.slots += p.slots & (~p.slots + 1);          // up to a power of two
    while (distinct + chunk_positions > p.slots / 2) p.slots *= 2;               // (both at most 2^32 - 1: no overflow)
    p.grow = p.slots != slots_now;
    p.grid = ceil_div(chunk_staged, kKmerTile);
    return p;
}
// the table a counter starts with: twice the hint, at least `floor_slots`
static inline uint64_t kmer_initial_slots(uint64_t expected_distinct, uint64_t floor_slots)
{
    const uint64_t want = std::min<uint64_t>(expected_distinct, kKmerCountLifetime);
    return plan_kmer_table(floor_slots, want, 0, 0).slots;
}

// ------------------------------------------------------------------------------ streamed search (search_stream_impl)
// The cut rule of bigsi_hip_search_stream and its _ranked and _scored siblings: the input goes out as device batches ("chunks") of
// consecutive sequences, kStreamSlots workspaces in flight.  A chunk holds at most `seqs` sequences and at most a position limit of
// k-mer positions, whichever it reaches first, and always at least one sequence.
//   - Position limit: exact (threshold 1.0) and scored streams take the small limit (2^20: gene-length queries ~1080 of 1 kbp; scored:
//     K5 + K6 of a chunk run beside the next chunk's row-AND -- more, smaller chunks), thresholded ones the large limit (2^22: the
//     counting kernel is ONE launch per chunk and every launch pays its tail -- 8192 x 1 kbp at 0.4 on 10 M x 100 k: 8 launches of
//     ~1080 queries 0.774 of peak by the kernel's clock, one launch of 8192 0.80).  The sequence cap still comes first for them: 4096
//     queries of 1 kbp are ~4.0 M positions, so 8192 of them go out as two chunks of 4096.
//   - An exact, unscored stream without BIGSI_RUN_FORCE_COUNTS (band_chunks) first cuts at the large limit and keeps that chunk if the
//     band sweep takes it (plan_band_sweep, and enough free device memory for its row lists: the loop's decision, not the planner's);
//     otherwise it cuts again at the small limit.
//   - An exact chunk that did not take the band sweep and has chunks behind it ends on a whole number of row-AND launches
//     (exact_launch_queries) once it holds two launches' worth: no chunk closes with a part launch (10 M x 100 k, 8192 x 1 kbp per
//     call: 8 chunks x 8 launches of 128 queries instead of 8 x (8 + a launch of 57)).
//   - 4096 sequences per chunk: host-visible over 1 M reads of 61 bp 1.04 / 1.41 / 1.51 / 1.45 G lookups/s at 1024 / 2048 / 4096 /
//     16384 reads per batch.  The workspaces are sized for that cap: an override may lower it, never raise it.
// Pinned by tests/c_host/stream_plan_host.cpp and tests/test_stream_plan_host.py; tests/test_gpu_stream_cuts.py reaches the cuts with
// small limits (bigsi_hip_stream_set_limits) and reads them back (bigsi_hip_stream_last_chunks).
constexpr uint64_t kStreamChunkPositions = 1ull << 20;
constexpr uint64_t kStreamLargeChunkPositions = 1ull << 22;
constexpr uint64_t kStreamChunkSeqs = 4096;
constexpr int kStreamSlots = 4;
struct StreamOverrides {            // bigsi_hip_stream_set_limits: 0 keeps the rule's value
    uint64_t chunk_positions = 0, large_chunk_positions = 0, chunk_seqs = 0;
};
struct StreamLimits {
    uint64_t small_pos, large_pos;      // position limit of a small chunk, of a large chunk
    uint64_t seqs;                      // sequences per chunk
    bool small_chunks;                  // a chunk of this stream takes the small limit (else the large one)
    bool band_chunks;                   // ... after the large one was tried for the band sweep
    uint64_t chunk_pos() const { return small_chunks ? small_pos : large_pos; }
};
static inline StreamLimits stream_limits(double threshold, bool scored, bool force_counts, const StreamOverrides &o = StreamOverrides())
{
    StreamLimits l;
    l.small_pos = o.chunk_positions ? o.chunk_positions : kStreamChunkPositions;
    l.large_pos = o.large_chunk_positions ? o.large_chunk_positions : kStreamLargeChunkPositions;
    l.seqs = o.chunk_seqs ? std::min(o.chunk_seqs, kStreamChunkSeqs) : kStreamChunkSeqs;
    l.small_chunks = threshold == 1.0 || scored;
    l.band_chunks = threshold == 1.0 && !scored && !force_counts;
    return l;
}

// The chunk that starts at sequence `next` < n_seqs: sequences [next, end), greedily while it holds at most limit_seqs sequences and
// limit_pos k-mer positions -- and at least one sequence, so that a sequence beyond the limit is a chunk of its own.  A sequence
// without a k-mer (shorter than k, or empty) adds nothing to what is compared with the limit and one position to `pos`.
struct StreamChunk {
    uint64_t end = 0;
    uint64_t pos = 0;          // sum of max(positions, 1) over the chunk
    uint64_t max_pos = 0;      // positions of its longest sequence
    bool bad_offsets = false;  // offsets[end + 1] < offsets[end]: the input is refused
};
static inline StreamChunk stream_chunk_end(const uint64_t *offsets, uint64_t n_seqs, uint64_t next, uint32_t k, uint64_t limit_pos, uint64_t limit_seqs)
{
    StreamChunk c;
    c.end = next;
    while (c.end < n_seqs && c.end - next < limit_seqs) {
        if (offsets[c.end + 1] < offsets[c.end]) { c.bad_offsets = true; return c; }
        const uint64_t len = offsets[c.end + 1] - offsets[c.end], n = len >= k ? len - k + 1 : 0;
        if (c.end > next && c.pos + n > limit_pos) break;
        c.pos += std::max<uint64_t>(n, 1);
        c.max_pos = std::max(c.max_pos, n);
        c.end++;
    }
    return c;
}

// sequences of a chunk cut at `n`, ended on whole row-AND launches of launch_q queries (see above)
static inline uint64_t stream_round_to_launches(uint64_t n, uint32_t launch_q, bool more_follow, bool exact, bool band)
{
    if (exact && !band && more_follow && launch_q && n >= 2ull * launch_q) return n / launch_q * launch_q;
    return n;
}

// ------------------------------------------------------------------------------ K4 hit lists (k_hits_totals, k_hits_write) and the export
// K4 works on items: an item is one 256-word chunk of one (sequence, shard) result vector, in (seq, shard, chunk) order, `nchunks`
// of them in all (the host keeps that below 2^31).  Workgroup g owns the `ipb` consecutive items [g ipb, (g + 1) ipb).
//   - At most kHitsOneGroupItems items (one or two gene-length queries: a latency-bound call) go to ONE workgroup, which needs
//     nobody's totals; on an unsharded buffer that workgroup takes k_hits_write's single-workgroup body (every thread a run of
//     consecutive words of a query) and, in a one-call search, writes the caller's pinned block itself.
//   - More items are spread over at most kHitsMaxGroups workgroups: ipb = ceil(nchunks / kHitsMaxGroups), groups = ceil(nchunks / ipb),
//     so that groups ipb >= nchunks > (groups - 1) ipb -- no workgroup is empty, the last one may be short.
// No items: one workgroup that owns nothing (the library does not launch K4 for an empty batch).
// The pinned block of an export carries the first export_spec hits along: kExportSpecPerSeq per sequence -- a read stream whose reads
// match a handful of samples each then never takes the slower fetch route --, at least kExportSpecMin, never more than the device
// lists hold, nor than kExportSpecMax.
// Pinned by tests/c_host/hits_plan_host.cpp and tests/test_hits_plan_host.py; tests/test_gpu_hit_lists.py reads the path a run took
// back through bigsi_hip_hits_last_path.
constexpr uint32_t kHitsMaxGroups = 1024;
constexpr uint32_t kHitsOneGroupItems = 16;
constexpr uint64_t kHitsInitialCapacity = 1ull << 16;      // entries the hit lists start with
constexpr uint64_t kExportSpecMin = 1024, kExportSpecPerSeq = 16, kExportSpecMax = 1ull << 20;
struct HitsPlan {
    uint32_t ipb = 1;           // items per workgroup
    uint64_t groups = 1;        // workgroups
    bool single = false;        // k_hits_write takes its single-workgroup body
};
static inline HitsPlan plan_hits(uint64_t nchunks, uint32_t n_shards = 1)
{
    HitsPlan p;
    if (nchunks > 0) {
        p.ipb = nchunks <= kHitsOneGroupItems ? (uint32_t)nchunks : (uint32_t)ceil_div(nchunks, (uint64_t)kHitsMaxGroups);
        p.groups = ceil_div(nchunks, p.ipb);
    }
    // (one workgroup means at most kHitsOneGroupItems items, hence at most that many chunks per vector: the kernel's own test)
    p.single = p.groups == 1 && n_shards == 1;
    return p;
}
static inline uint64_t export_spec(uint64_t n_seqs, uint64_t capacity)
{
    return std::min<uint64_t>(std::max<uint64_t>(kExportSpecMin, kExportSpecPerSeq * n_seqs), std::min<uint64_t>(capacity, kExportSpecMax));
}

}  // namespace bigsi
