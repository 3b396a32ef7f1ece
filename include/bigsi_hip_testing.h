/*
 * bigsi_hip_testing.h -- entry points and flags of libbigsi_hip.so that are exported but NOT part of the advertised boundary
 * (include/bigsi_hip.h): what the test-suite and the A/B scripts need to drive the library from outside.
 *
 *   - EXCHANGE-BY-CALLER: a host that brings its own collective instead of the library's RCCL communicator -- here
 *     torch.distributed over gloo, so that several ranks can share the one GPU of a test box (RCCL refuses two ranks on one
 *     device): caller-owned streams and result buffers, compaction of a buffer the caller gathered.
 *   - BIGSI_RUN_* flags that force a route (same results by construction; tests/test_gpu_parity.py proves it).
 * A production binder needs none of this.
 */
#ifndef BIGSI_HIP_TESTING_H
#define BIGSI_HIP_TESTING_H

#include "bigsi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* test / A-B flags: same results, different route (tests/test_gpu_parity.py, scripts/ab_*.py); not for production callers */
#define BIGSI_RUN_K1_GLOBAL 4u   /* take the multi-launch K1 (global-memory dedupe table) whatever the query lengths */
#define BIGSI_RUN_NO_SORT 16u    /* stream each query's rows in hash order instead of address order */
/* (128u was BIGSI_RUN_NO_WAITING in rounds 2-3: the read kernel's bounded wait between workgroups; the kernel no longer waits) */
#define BIGSI_RUN_ONE_STREAM 256u /* one-launch read path: this run goes to the index stream instead of the next of the three read
                                    streams, so that consecutive launches do NOT overlap -- a kernel's own duration is then what it
                                    takes alone on the device (bench.py: roofline.frac of read workloads) */
#define BIGSI_RUN_WEAK_FINGERPRINT 64u /* one-launch read path: 1-bit k-mer fingerprints, so that the dedupe takes its exact
                                          pairwise route (otherwise reached only on a 2^-32 fingerprint collision) */

#define BIGSI_RUN_BAND_SWEEP 512u /* exact runs: take the band sweep (one column segment of every query per launch, plan_band_sweep)
                                     whatever the batch's size and the share of repeated rows; declined with BIGSI_RUN_EARLY_EXIT,
                                     BIGSI_RUN_NO_SORT and on the counting path */

/* Run this index's kernels and copies on a caller-owned hipStream_t (e.g. torch's current stream, so
 * that RCCL collectives issued by the caller are ordered after them).  NULL restores the private stream.
 * With a caller-owned stream set, every kernel of the index goes to that one stream (see STREAMS in bigsi_hip.h). */
int bigsi_hip_set_stream(bigsi_hip_index *ix, void *hip_stream);

/* Write the per-sample bit vectors of later runs (the exact AND, or the hit mask of a thresholded run) into caller-owned device
 * memory (e.g. this rank's slot of an all-gather buffer) instead of the batch's own buffer.  NULL = keep the own buffer.
 * Counters always stay in the batch: they are never exchanged. */
int bigsi_hip_batch_set_outputs(bigsi_hip_batch *b, void *d_bitmaps);
/* Width, in columns, of the per-sample result vectors of later runs (default 0 = the index's num_cols).  The shards of one
 * index all set the group's shard width here, so that uneven shards still exchange buffers of ONE geometry (strides, word
 * counts); needs cols <= col_capacity.  Columns beyond the shard's own num_cols read as zero. */
int bigsi_hip_batch_set_result_cols(bigsi_hip_batch *b, uint64_t cols);

/* EXCHANGE-BY-CALLER.  Multi-GPU assembly: compact hits from result buffers gathered from n_shards column shards (device pointer,
 * layout [shard][seq][stride] with this batch's strides; colour = shard * shard_cols + local column).
 * compact_gathered* are asynchronous, also for the host: they are queued (on the gather stream, below) behind this batch's
 * run through an event, never by waiting for it -- call them after the RCCL all-gather, which the caller issues on the
 * same stream; fetch_gathered_hits synchronises and copies out, same format as fetch_hits. */
/* Run this batch's gathered compaction (and the copies of fetch_gathered_hits) on a caller-owned hipStream_t -- typically
 * the stream the collective is issued under, so that all-gather + compaction of one batch overlap the row-AND kernels of
 * the next batch on the index's stream.  NULL = the index's stream. */
int bigsi_hip_batch_set_gather_stream(bigsi_hip_batch *b, void *hip_stream);
/* Exact runs: every hit's count is the query's number of unique k-mers.  After a thresholded run: BIGSI_ERR_STATE, nothing queued
 * (its exchange is compact_gathered_masks, which accepts exact runs too). */
int bigsi_hip_batch_compact_gathered(bigsi_hip_batch *b, const void *d_gathered, uint32_t n_shards, uint64_t shard_cols);
/* Thresholded search over column shards without moving per-sample counters: the counting kernel also leaves each
 * shard's hit mask (1 bit per sample: count >= min_kmers) in the bitmap output (bigsi_hip_batch_set_outputs), which is what
 * gets all-gathered.  compact_gathered_masks compacts the gathered masks -- identically on every rank -- and fills each
 * hit's count from THIS rank's counters when the hit lies in shard `own_shard`, 0 otherwise; the caller then sums the
 * count arrays of all ranks (one fixed-size all-reduce over the buffer given to set_gathered_hit_outputs). */
int bigsi_hip_batch_compact_gathered_masks(bigsi_hip_batch *b, const void *d_gathered_masks, uint32_t n_shards, uint64_t shard_cols,
                                           uint32_t own_shard);
/* Put the gathered hit lists (colours, counts: uint32[capacity] each) into caller-owned device memory.  With caller-owned
 * buffers fetch_gathered_hits reports BIGSI_ERR_CAPACITY instead of growing them. */
int bigsi_hip_batch_set_gathered_hit_outputs(bigsi_hip_batch *b, void *d_colours, void *d_counts, uint64_t capacity);

/* MEASUREMENT (bench.py, scripts/measure.py).
 * bigsi_hip_insert_columns with the filters already in device memory (no staging copy: what prices the transpose kernel alone).
 * A 16-byte aligned pointer and pitch take the tiled transpose; anything else the column-at-a-time route.  d_blooms spans
 * n * bloom_stride_bytes bytes: the tiled route loads 16 bytes at a time, inside a filter's pitch but up to 15 bytes behind its
 * ceil(num_rows/8); what those bytes, and the bits of the last byte behind row num_rows - 1, hold reaches no row. */
int bigsi_hip_insert_columns_device(bigsi_hip_index *ix, uint64_t col0, uint64_t n, const void *d_blooms, uint64_t bloom_stride_bytes);
/* Same-box calibration: achieved GB/s of bare row streams over this index's matrix -- a kernel with no BIGSI code, the load
 * pattern of the row-AND kernels (one wavefront per 1 KiB column segment, 16 B per lane, 8 loads in flight) -- over n_queries
 * lists of rows_per_query rows, uniform random (sorted = 0: what the counting kernel sees) or ascending (1: the exact kernel's
 * address-ordered lists); launches of `wgs` workgroups (0 = the library's own launch size); median of `reps` passes.
 * Lets a bench line state its fraction of what THIS box delivers (boxes differ by several per cent at identical clocks). */
int bigsi_hip_probe_rows(bigsi_hip_index *ix, uint32_t rows_per_query, uint32_t n_queries, uint32_t sorted, uint32_t wgs, uint32_t reps,
                         double *gbps, double *launch_ms);

/* K-MER COUNTER (include/bigsi_hip_kmercount.h): the staging chunk of later adds, in bytes (at least 64), and the slot count a
 * reset starts from (a power of two, at least 64); 0 keeps the library's own value.  With small values a test reaches a chunk cut
 * and several table growths with a few kilobytes of input; results do not depend on either.  BIGSI_ERR_STATE on a counter that
 * holds anything: call it right after create or reset (an empty counter takes the new slot count at once). */
struct bigsi_hip_kmer_counter;
int bigsi_hip_kmer_counter_set_limits(struct bigsi_hip_kmer_counter *c, uint64_t chunk_bytes, uint64_t initial_slots);

/* WINDOWED SEARCH (include/bigsi_hip_window.h): window starts per segment of later sweeps of this index (0: the planner's own
 * choice) and the cap, in bytes, on the per-segment maxima a sweep may leave (0: the library's 2 GiB).  With 64 starts per segment
 * a test reaches segment boundaries with a few hundred positions, and with a small cap the refusal; results do not depend on the
 * first.  BIGSI_ERR_INVALID for a NULL index or starts_per_segment >= 2^31. */
int bigsi_hip_window_set_limits(bigsi_hip_index *ix, uint64_t starts_per_segment, uint64_t partial_bytes_cap);

/* BAND SWEEP (plan_band_sweep): address windows per band and column segments per launch (1 or 2) of later exact runs of this index
 * that take the route; 0 keeps the planner's own value.  With many windows a test reaches empty windows and the hand-over of the
 * accumulator between launches on a few hundred rows; results do not depend on either.  BIGSI_ERR_INVALID for a NULL index, more
 * than 65536 windows or more than 2 segments. */
int bigsi_hip_band_set_limits(bigsi_hip_index *ix, uint32_t windows, uint32_t segments_per_launch);

/* STREAMED SEARCH (stream_limits, stream_chunk_end): the k-mer positions of a small chunk (the library's 2^20: exact and scored
 * streams) and of a large chunk (2^22: thresholded streams, and the exact chunk that is tried for the band sweep), and the sequences per
 * chunk (4096), of later bigsi_hip_search_stream / _ranked / _scored calls on this index; 0 keeps the library's value.  With small
 * values a test reaches chunk cuts and the reuse of the four workspaces with a few hundred short queries; results do not depend on
 * any of the three.  BIGSI_ERR_INVALID for a NULL index or chunk_seqs above 4096 (the workspaces are sized for that). */
int bigsi_hip_stream_set_limits(bigsi_hip_index *ix, uint64_t chunk_positions, uint64_t large_chunk_positions, uint64_t chunk_seqs);
/* The chunks the last streamed search on this index launched, in order: *n of them, first[i] the index of chunk i's first sequence,
 * band[i] != 0 when the stream gave the chunk to the band sweep.  A stream of no sequences, and one refused before its first chunk
 * (the argument checks of the three entry points included), report none; a stream that failed later the chunks launched until
 * then.  capacity < *n is a sizing call: BIGSI_ERR_CAPACITY, *n set, nothing written (first and band may then be NULL). */
int bigsi_hip_stream_last_chunks(bigsi_hip_index *ix, uint64_t *first, uint8_t *band, uint64_t capacity, uint64_t *n);

/* HIT LISTS AND THE EXPORT (plan_hits, export_spec): the path the LAST run of a batch took through the hit-list compaction
 * (k_hits_totals / k_hits_write), the export into pinned memory and bigsi_batch_collect.  Results never depend on it; a test built
 * for one path asserts it here first.  The call only reads what the run, its fetches and its collect left on the host: it queues
 * nothing and waits for nothing.
 *   groups, items_per_group  k_hits_write's grid and the items a workgroup owns (0, 0: K4 did not run -- a one-launch read run, or a
 *                            run without hit lists)
 *   single_workgroup         k_hits_write took its single-workgroup body
 *   inline_export            the run's own kernel wrote the caller's pinned block (k_hits_write's single-workgroup body, or the read
 *                            kernel of a one-read call) -- there was no export kernel
 *   rewrites                 write passes repeated after the lists were grown (the read kernel: whole launches repeated)
 *   exp_spec                 hits the export carried along (0: the run exported nothing)
 *   collect_fetch            the one-call search took its results by the fetch route, not from the pinned block
 *   one_launch               the run was the one-launch read kernel (k_reads_fused; a one-call search then exports with k_export_reads)
 * `kind` says what `owner` is: a bigsi_hip_batch, a bigsi_hip_index (its one-call workspace: the last bigsi_hip_search_batch) or a
 * bigsi_hip_group_batch (member 0, whose gathered lists the host reads).  BIGSI_ERR_INVALID for a NULL argument or an unknown kind,
 * BIGSI_ERR_STATE when there is no such batch or it has not run. */
typedef struct bigsi_hip_hits_path {
    uint32_t groups, items_per_group, single_workgroup, inline_export, rewrites, exp_spec, collect_fetch, one_launch;
} bigsi_hip_hits_path;
#define BIGSI_HITS_PATH_OF_BATCH 0u
#define BIGSI_HITS_PATH_OF_INDEX 1u
#define BIGSI_HITS_PATH_OF_GROUP_BATCH 2u
int bigsi_hip_hits_last_path(const void *owner, uint32_t kind, bigsi_hip_hits_path *out);

/* THE ROW-AND'S ROUTE (k1_plan, plan_row_and, plan_band_sweep, sort_rows_block): how the LAST run of a batch went through K1, the
 * row sort and the row-AND launches.  Results never depend on it; a test built for one route asserts it here first
 * (tests/knockout_cases.py).  bigsi_batch_run fills the record from the plans it holds anyway; the call only reads it: it queues
 * nothing and waits for nothing.  `owner` and `kind` as for bigsi_hip_hits_last_path, and the same errors.
 *   k1_route                 0 explicit k-mers, 1 one wavefront per query, 2 the LDS route (k_kmerize_lds), 3 the global route
 *   band_taken, band_windows, band_launches   the band sweep (k_and_exact_band) and its launches; 0, 0, 0: plan_row_and's launches
 *   slices, block, tiles, chunk_q, n_launches  plan_row_and's answer for the whole batch
 *   last_slices, last_block, last_unroll       its last launch (a chunked batch's tail is planned again: RowAndPlan::launch)
 *   sorted_by                who made the address-ordered row list K2 streamed: BIGSI_SORTED_BY_*
 *   early_exit               BIGSI_RUN_EARLY_EXIT reached the kernel
 *   preset_by                who set the result words a sliced exact run ANDs into: 0 nobody (not sliced), 1 K1, 2 a memset
 *   zero_copy                K1 read the sequences in place from the caller's pinned staging (a one-call search)
 *   k1_parts                 workgroups per query of K1: 8 where k_kmerize_lds spread a query's hashing (`parts`), else 1
 *   k1_arg_bytes             the instance that took the ONE sequence of a one-call search by value in its kernel arguments (SeqArg):
 *                            96 (k_reads_fused), 1024 or 3072 (k_kmerize_lds); 0: K1 read the sequences from memory
 * A one-launch read run (k_reads_fused) fills k1_parts (1) and k1_arg_bytes and leaves the rest of the record zero. */
typedef struct bigsi_hip_row_and_path {
    uint32_t k1_route, band_taken, band_windows, band_launches, slices, block, tiles, chunk_q, n_launches, last_slices, last_block,
        last_unroll, sorted_by, early_exit, preset_by, zero_copy, k1_parts, k1_arg_bytes;
} bigsi_hip_row_and_path;
#define BIGSI_SORTED_BY_NONE 0u
#define BIGSI_SORTED_BY_K1 1u
#define BIGSI_SORTED_BY_SORT256 2u
#define BIGSI_SORTED_BY_SORT1024 3u
int bigsi_hip_batch_last_row_and(const void *owner, uint32_t kind, bigsi_hip_row_and_path *out);
/* The row list K2 streamed for sequence `seq` in the last run of `b` -- num_unique x num_hashes row ids, `capacity` entries at
 * least -- and the shift it is bucket-ordered by (ascending in row >> shift): per query sort_shift(m, slots of the query's dedupe
 * table) on K1's LDS route, sort_shift(m, 8192) for k_sort_rows.  One device-to-host copy, no kernel.  BIGSI_ERR_STATE when the
 * last run made no sorted list, BIGSI_ERR_RANGE / BIGSI_ERR_CAPACITY as bigsi_hip_batch_fetch_rows. */
int bigsi_hip_batch_fetch_rows_sorted(bigsi_hip_batch *b, uint32_t seq, uint64_t *rows, uint64_t capacity, uint32_t *shift);
/* K1's two per-position maps of sequence `seq` as the last run of `b` left them, num_kmers entries each, `capacity` at least:
 * rep[p] the first position that holds position p's k-mer, pos_unique[p] the index of that k-mer among the sequence's unique k-mers
 * (what the presence strings expand by).  Either pointer may be NULL.  One device-to-host copy per array, no kernel.
 * BIGSI_ERR_STATE on a batch of explicit k-mers (its K1 dedupes nothing), BIGSI_ERR_RANGE / BIGSI_ERR_CAPACITY as
 * bigsi_hip_batch_fetch_rows. */
int bigsi_hip_batch_fetch_positions(bigsi_hip_batch *b, uint32_t seq, uint32_t *rep, uint32_t *pos_unique, uint64_t capacity);

/* THE TOP-N SELECTION ON CALLER DATA (k_rank_select; its peer for K6 is bigsi_hip_score_presence): no index, no batch.  For n_seqs
 * queries the call stages
 *   hits        uint64[n_seqs][stride_words], row format (column 8b + j of a word at bit 8b + 7 - j), of which the first wv words of a
 *               query are its result (wv <= stride_words);
 *   counters    uint16 (counter_bytes 2) or uint32 (4) [n_seqs][64 * stride_words], one per column, or NULL for an exact run (then
 *               num_unique and min_kmers are not read and may be NULL); the kernel reads a counter only where the column is a hit;
 *   num_unique, min_kmers   uint32[n_seqs];
 *   excluded    uint64[wv] in row format, shared by all queries, or NULL;
 * launches the instance and the grid a limited search launches (one workgroup per query, the same argument meaning as rank_select()
 * in bigsi_hip.hip), waits, and copies all of [n_seqs][stride_words] back into `out`.  in_place = 0: the kernel writes a second
 * buffer, preset with what `out` holds on entry -- so a caller sees which words the kernel left alone; in_place != 0: the kernel
 * trims the staged hits themselves (out == hits on the device: a group member's slot of the gather buffer).
 * BIGSI_ERR_INVALID, before any device work, for hits or out NULL, wv > stride_words, counters with a counter_bytes other than 2 or 4
 * or without num_unique / min_kmers, and limit == 0. */
int bigsi_hip_rank_select_arrays(int device, const uint64_t *hits, uint64_t stride_words, uint32_t wv, uint32_t n_seqs, const void *counters,
                                 uint32_t counter_bytes, const uint32_t *num_unique, const uint32_t *min_kmers, const uint64_t *excluded,
                                 uint32_t limit, uint32_t in_place, uint64_t *out);

#ifdef __cplusplus
}
#endif
#endif /* BIGSI_HIP_TESTING_H */
