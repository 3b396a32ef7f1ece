/*
 * bigsi_hip_tally.h -- query-set tally of libbigsi_hip.so: over a whole set of query sequences, how many of them hit each sample and
 * how many k-mers those hits found -- summed on the device, two numbers per sample leaving it.
 *
 * Part of the QUERY layer of the C ABI (include/bigsi_hip.h): entry points in that header's conventions (return codes,
 * bigsi_hip_last_error, one thread per handle, the row format).  A header of its own because bigsi_hip.h is kept to 60 entry points
 * (tests/test_abi_and_host.py pins it): the Python binding lists these in TALLY_SIGNATURES.
 */
#ifndef BIGSI_HIP_TALLY_H
#define BIGSI_HIP_TALLY_H

#include "bigsi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What is summed.  For sequence i of the set, k and a threshold t <= 1: u_i its distinct k-mers (a search's num_unique), mk_i =
 * max(ceil((double)u_i * t), 0) (a search's min_kmers), c_i[s] the number of those k-mers whose h rows all have column s set, and
 * hit_i[s] = (c_i[s] >= mk_i) for s < num_cols -- the hits bigsi_hip_search_batch reports.  A sequence with u_i == 0 (shorter than k)
 * contributes nothing.  Then
 *     queries_hit[s] = sum_i hit_i[s]
 *     kmers_found[s] = sum_i hit_i[s] * c_i[s]          (t == 1.0: a hit has c = u_i)
 *     totals[0] = sequences counted (u_i > 0)            totals[1] = sum of u_i over them
 *     totals[2] = sequences skipped (u_i == 0)           totals[3] = counted sequences with at least one hit
 * All of them uint64 sums of integers: bit-identical from run to run and under any cut of the set into batches or calls.
 *
 *   tally_create     device accumulators, zeroed, for the index's num_cols at this moment.  The tally belongs to the index: destroy
 *                    it before bigsi_hip_close.  An index whose num_cols, num_rows or num_hashes have changed since gets
 *                    BIGSI_ERR_STATE from every call but destroy.
 *   tally_reset      zeroes the accumulators (and makes a tally usable again after a failed tally_add_stream).
 *   tally_add_batch  adds a batch of this index whose last run was made with BIGSI_RUN_SKIP_COMPACT: its result vectors (and, below
 *                    threshold 1, its counters) are summed by two kernels queued on the stream the run finished on -- asynchronous,
 *                    no host wait.  The batch's completion event is recorded again behind them, so bigsi_hip_batch_reload,
 *                    bigsi_hip_batch_run and bigsi_hip_batch_destroy directly afterwards are safe without any synchronisation by
 *                    the caller: whatever waited for the run now waits for the tally too.  BIGSI_ERR_STATE for a batch of another
 *                    index, one that has not run, one whose last run built hit lists (no BIGSI_RUN_SKIP_COMPACT, or the one-launch
 *                    read kernel), one with a result limit, with caller-owned bit vectors (bigsi_hip_batch_set_outputs), a result
 *                    width (bigsi_hip_batch_set_result_cols) or a communicator.
 *   tally_add_stream any number of host sequences (the arguments of bigsi_hip_search_stream): cut into device batches of at most
 *                    BIGSI_TALLY_CHUNK_SEQS sequences, BIGSI_TALLY_CHUNK_POSITIONS k-mer positions and, below threshold 1,
 *                    BIGSI_TALLY_COUNTER_BYTES of dense counters (n_seqs * padded columns * 4 bytes: the counting run's allocation
 *                    is bounded whatever the width of the index) -- at least one sequence each -- that alternate over two
 *                    workspaces of the index: the next one is staged while the current one runs.  Returns when everything has been
 *                    queued and the input is no longer read.  The workspaces are created at the first call and live until
 *                    bigsi_hip_close.  On a failure they are destroyed and the tally is marked unusable (every call but reset and
 *                    destroy: BIGSI_ERR_STATE) -- chunks before the failing one may have been added; tally_reset starts over.
 *   tally_fetch      waits for everything added so far and copies the num_cols entries of both vectors and totals[4] out; the
 *                    accumulators keep their values (a second fetch returns the same).  BIGSI_ERR_CAPACITY when capacity <
 *                    num_cols: nothing is written.
 * BIGSI_ERR_INVALID: a NULL argument, and what a batch's arguments are refused for.  All calls only read the index: ipc and view
 * handles are fine.  There are no group twins. */
#define BIGSI_TALLY_CHUNK_SEQS 4096u
#define BIGSI_TALLY_CHUNK_POSITIONS (1u << 20)
#define BIGSI_TALLY_COUNTER_BYTES (2ull << 30)

typedef struct bigsi_hip_tally bigsi_hip_tally;
int bigsi_hip_tally_create(bigsi_hip_index *ix, bigsi_hip_tally **out);
int bigsi_hip_tally_destroy(bigsi_hip_tally *t);
int bigsi_hip_tally_reset(bigsi_hip_tally *t);
int bigsi_hip_tally_add_batch(bigsi_hip_tally *t, bigsi_hip_batch *b);
int bigsi_hip_tally_add_stream(bigsi_hip_tally *t, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold);
int bigsi_hip_tally_fetch(bigsi_hip_tally *t, uint64_t *queries_hit, uint64_t *kmers_found, uint64_t capacity, uint64_t totals[4]);

#ifdef __cplusplus
}
#endif

#endif /* BIGSI_HIP_TALLY_H */
