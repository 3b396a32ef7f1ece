// CPU pin of the streamed search's cut rule in bigsi_amd/csrc/bigsi_launch.hpp (stream_limits, stream_chunk_end,
// stream_round_to_launches, exact_launch_queries), compiled here as plain host C++.  tests/test_stream_plan_host.py loads it and
// compares it with the Python restatement in tests/stream_ref.py.
// Test infrastructure only: nothing in the product loads this file.
#include "../../bigsi_amd/csrc/bigsi_launch.hpp"

extern "C" {

// out[]: small_pos, large_pos, seqs, small_chunks, band_chunks, chunk_pos()
void stream_host_limits(double threshold, int scored, int force_counts, uint64_t chunk_positions, uint64_t large_chunk_positions, uint64_t chunk_seqs,
                        uint64_t *out)
{
    bigsi::StreamOverrides o;
    o.chunk_positions = chunk_positions;
    o.large_chunk_positions = large_chunk_positions;
    o.chunk_seqs = chunk_seqs;
    const bigsi::StreamLimits l = bigsi::stream_limits(threshold, scored != 0, force_counts != 0, o);
    const uint64_t v[6] = {l.small_pos, l.large_pos, l.seqs, l.small_chunks, l.band_chunks, l.chunk_pos()};
    for (int i = 0; i < 6; i++) out[i] = v[i];
}

// out[]: end, pos, max_pos, bad_offsets
void stream_host_chunk_end(const uint64_t *offsets, uint64_t n_seqs, uint64_t next, uint32_t k, uint64_t limit_pos, uint64_t limit_seqs, uint64_t *out)
{
    const bigsi::StreamChunk c = bigsi::stream_chunk_end(offsets, n_seqs, next, k, limit_pos, limit_seqs);
    out[0] = c.end;
    out[1] = c.pos;
    out[2] = c.max_pos;
    out[3] = c.bad_offsets;
}

uint64_t stream_host_round(uint64_t n, uint32_t launch_q, int more_follow, int exact, int band)
{
    return bigsi::stream_round_to_launches(n, launch_q, more_follow != 0, exact != 0, band != 0);
}

uint32_t stream_host_launch_queries(uint64_t wv) { return bigsi::exact_launch_queries(wv); }

// the shipped constants: positions of a small chunk, of a large chunk, sequences per chunk, workspaces in flight
void stream_host_constants(uint64_t *out)
{
    out[0] = bigsi::kStreamChunkPositions;
    out[1] = bigsi::kStreamLargeChunkPositions;
    out[2] = bigsi::kStreamChunkSeqs;
    out[3] = (uint64_t)bigsi::kStreamSlots;
}

}
