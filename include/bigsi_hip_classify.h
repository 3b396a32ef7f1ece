/*
 * bigsi_hip_classify.h -- read classification of libbigsi_hip.so: for every query sequence, which GROUP of samples it belongs to --
 * the hits of each group summed per query on the device, a fixed 48-byte record per query leaving it however many samples were hit.
 *
 * Part of the QUERY layer of the C ABI (include/bigsi_hip.h): entry points in that header's conventions (return codes,
 * bigsi_hip_last_error, one thread per handle, the row format).  A header of its own because bigsi_hip.h is kept to 60 entry points
 * (tests/test_abi_and_host.py pins it): the Python binding lists these in CLASSIFY_SIGNATURES.
 */
#ifndef BIGSI_HIP_CLASSIFY_H
#define BIGSI_HIP_CLASSIFY_H

#include "bigsi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What is computed.  Inputs: group_of[num_cols] (uint32: below n_groups, or BIGSI_CLASSIFY_NONE for a column in no group), 1 <=
 * n_groups <= BIGSI_CLASSIFY_MAX_GROUPS, k and a threshold t <= 1.  For sequence i the quantities are those of bigsi_hip_tally.h: u_i
 * its distinct k-mers, mk_i = max(ceil((double)u_i * t), 0), c_i[s] the number of those k-mers whose h rows all have column s set, and
 * hit_i[s] = (c_i[s] >= mk_i) for s < num_cols.  Per group g:
 *     samples_hit_i[g] = number of hit columns of g
 *     found_i[g]       = max of c_i[s] over the hit columns of g          (t == 1.0: every hit has c = u_i)
 *     colour_i[g]      = the LOWEST hit colour of g that holds that maximum
 * A group is HIT when samples_hit_i[g] > 0, not when found_i[g] > 0: at t <= 0 every grouped column is a hit, those with count 0
 * included.  Hit groups are ordered by found descending, ties to the lower group id; best_* is the first group in that order and
 * second_* the next.  An absent place has group and colour BIGSI_CLASSIFY_NONE, found 0, samples 0.  A sequence with u_i == 0 (shorter
 * than k) gets an all-absent record with num_unique = min_kmers = 0, whatever its result vector holds.  Bits behind num_cols are never
 * trusted, and the pad word of a batch's padded result vector is never read.  Everything is integer max / add: the records are
 * bit-identical from run to run and under any cut of the input into chunks.
 *
 *   classify_batch   takes a batch of this index whose last run was made with BIGSI_RUN_SKIP_COMPACT (its counters, below threshold 1,
 *                    dense or BIGSI_RUN_SPARSE_COUNTS): uploads group_of, queues k_classify_groups on the stream the run finished
 *                    on, records the batch's completion event again behind the kernel -- so bigsi_hip_batch_reload,
 *                    bigsi_hip_batch_run and bigsi_hip_batch_destroy directly afterwards are safe without any synchronisation by the
 *                    caller --, downloads the batch's n_seqs records and returns.  BIGSI_ERR_STATE for a batch of another index, one
 *                    that has not run, one whose last run built hit lists (no BIGSI_RUN_SKIP_COMPACT, or the one-launch read kernel),
 *                    one with a result limit, with caller-owned bit vectors (bigsi_hip_batch_set_outputs), a result width
 *                    (bigsi_hip_batch_set_result_cols) or a communicator, or whose num_hashes changed since the run.
 *                    BIGSI_ERR_CAPACITY when capacity < n_seqs: nothing is written.
 *   classify_stream  any number of host sequences (the arguments of bigsi_hip_search_stream): cut into device batches by the tally's
 *                    rule (BIGSI_TALLY_CHUNK_SEQS, BIGSI_TALLY_CHUNK_POSITIONS, BIGSI_TALLY_COUNTER_BYTES; include/bigsi_hip_tally.h)
 *                    that alternate over two workspaces of the index of the call's own: the next chunk is staged while the current
 *                    one runs.  records takes n_seqs entries, sequence s0 + j of a chunk at records[s0 + j].  A chunk without a
 *                    k-mer position never goes to the device: its records are written empty on the host.  The workspaces are created
 *                    at the first call and live until bigsi_hip_close.  On a failure they are destroyed and the error is returned;
 *                    records is then unspecified.
 * BIGSI_ERR_INVALID: a NULL argument, n_entries != num_cols, n_groups outside 1 .. BIGSI_CLASSIFY_MAX_GROUPS, a group_of value that is
 * neither below n_groups nor BIGSI_CLASSIFY_NONE (the message names the column), k == 0, n_seqs == 0, descending offsets, a threshold
 * above 1.  BIGSI_ERR_STATE: an index without columns.  The calls only read the index: ipc and view handles are fine.  There are no
 * group twins. */
#define BIGSI_CLASSIFY_NONE 0xFFFFFFFFu
#define BIGSI_CLASSIFY_MAX_GROUPS 4096u

typedef struct bigsi_hip_classify_record {
    uint32_t num_unique, min_kmers, groups_hit, samples_hit;      /* samples_hit: hit columns that are in any group */
    uint32_t best_group, best_found, best_colour, best_samples_hit;
    uint32_t second_group, second_found, second_colour, second_samples_hit;
} bigsi_hip_classify_record;

int bigsi_hip_classify_batch(bigsi_hip_batch *b, const uint32_t *group_of, uint64_t n_entries, uint32_t n_groups,
                             bigsi_hip_classify_record *records, uint64_t capacity);
int bigsi_hip_classify_stream(bigsi_hip_index *ix, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold,
                              const uint32_t *group_of, uint64_t n_entries, uint32_t n_groups, bigsi_hip_classify_record *records);

#ifdef __cplusplus
}
#endif

#endif /* BIGSI_HIP_CLASSIFY_H */
