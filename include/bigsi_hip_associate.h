/*
 * bigsi_hip_associate.h -- group association of libbigsi_hip.so: for every query sequence (a unitig, a gene, a probe of a panel), how
 * many samples of each phenotype GROUP hold it -- every group's count, the zeros included, taken on the device by mask-and-popcount
 * over the result vectors; n_groups + 4 integers per query leave it however many samples were hit.
 *
 * Part of the QUERY layer of the C ABI (include/bigsi_hip.h): entry points in that header's conventions (return codes,
 * bigsi_hip_last_error, one thread per handle, the row format).  A header of its own because bigsi_hip.h is kept to 60 entry points
 * (tests/test_abi_and_host.py pins it): the Python binding lists these in ASSOCIATE_SIGNATURES.
 */
#ifndef BIGSI_HIP_ASSOCIATE_H
#define BIGSI_HIP_ASSOCIATE_H

#include "bigsi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What is computed.  Inputs: group_of[num_cols] (uint32: below n_groups, or BIGSI_ASSOCIATE_NONE for a column in no group -- a
 * partition of the columns, as bigsi_hip_classify.h takes it), 1 <= n_groups <= BIGSI_ASSOCIATE_MAX_GROUPS, k and a threshold t <= 1.
 * For sequence i the quantities are those of bigsi_hip_tally.h / bigsi_hip_classify.h: u_i its distinct k-mers, mk_i =
 * max(ceil((double)u_i * t), 0), c_i[s] the number of those k-mers whose h rows all have column s set, and hit_i[s] = (c_i[s] >= mk_i)
 * for s < num_cols.  Then
 *     counts[i * n_groups + g] = number of columns s < num_cols with hit_i[s] and group_of[s] == g          (uint32)
 *     info[i] = { num_unique = u_i, min_kmers = mk_i, samples_hit = hit columns (grouped or not),
 *                 grouped_hit = sum over g of counts[i * n_groups + g] }                                     (4 x uint32)
 * A sequence with u_i == 0 (shorter than k) gets all zeros, min_kmers included, whatever its result vector holds.  At t <= 0 every
 * column is a hit: counts[i][g] is the size of group g and samples_hit = num_cols.  Bits behind num_cols are never trusted, and the
 * pad word of a batch's padded result vector is never read.  A group without a member is legal here and counts 0.  Everything is
 * integer AND / popcount / add: the results are bit-identical from run to run and under any cut of the input into chunks.
 *
 * Why 64 groups.  The count kernel reads one mask word per group and result word: n_groups x ceil(num_cols / 64) x 8 bytes of masks
 * per query, from cache -- 0.8 MB at 100 k columns, 4.9 MB at 600 k.  That is the right trade for phenotype groups (cases / controls,
 * a handful of lineages) on hit-dense input, where its cost does not depend on the number of hits.  A finer partition -- hundreds of
 * species -- belongs to the group_of-lookup design of bigsi_hip_classify.h, whose cost follows the hits and not the groups.  64 is a
 * design limit, not a measured one.
 *
 *   associate_batch  takes a batch of this index whose last run was made with BIGSI_RUN_SKIP_COMPACT (exact or counting, dense or
 *                    BIGSI_RUN_SPARSE_COUNTS: no counter is read): uploads group_of, queues k_group_masks and k_group_counts on the
 *                    stream the run finished on, records the batch's completion event again behind them -- so
 *                    bigsi_hip_batch_reload, bigsi_hip_batch_run and bigsi_hip_batch_destroy directly afterwards are safe without
 *                    any synchronisation by the caller --, downloads the batch's n_seqs x n_groups counts and n_seqs infos and
 *                    returns.  BIGSI_ERR_STATE for a batch that has not run, one whose last run built hit lists (no
 *                    BIGSI_RUN_SKIP_COMPACT, or the one-launch read kernel), one with a result limit, with caller-owned bit vectors
 *                    (bigsi_hip_batch_set_outputs), a result width (bigsi_hip_batch_set_result_cols) or a communicator, or whose
 *                    num_hashes or num_cols changed since the run.  BIGSI_ERR_CAPACITY when capacity (in sequences, of both
 *                    outputs) < n_seqs: nothing is written.
 *   associate_stream any number of host sequences (the arguments of bigsi_hip_search_stream): cut into device batches by the tally's
 *                    rule (BIGSI_TALLY_CHUNK_SEQS, BIGSI_TALLY_CHUNK_POSITIONS, BIGSI_TALLY_COUNTER_BYTES; include/bigsi_hip_tally.h)
 *                    that alternate over two workspaces of the index of the call's own: the next chunk is staged while the current
 *                    one runs.  counts takes n_seqs x n_groups entries and info n_seqs, sequence s0 + j of a chunk at index s0 + j.
 *                    A chunk without a k-mer position never goes to the device: its outputs are written as zeros on the host.  The
 *                    workspaces are created at the first call and live until bigsi_hip_close.  On a failure they are destroyed and
 *                    the error is returned; the outputs are then unspecified.
 * BIGSI_ERR_INVALID: a NULL argument, n_entries != num_cols, n_groups outside 1 .. BIGSI_ASSOCIATE_MAX_GROUPS, a group_of value that
 * is neither below n_groups nor BIGSI_ASSOCIATE_NONE (the message names the column), k == 0, n_seqs == 0, descending offsets, a
 * threshold above 1.  BIGSI_ERR_STATE: an index without columns.  The calls only read the index: ipc and view handles are fine.  There
 * are no group twins. */
#define BIGSI_ASSOCIATE_NONE 0xFFFFFFFFu
#define BIGSI_ASSOCIATE_MAX_GROUPS 64u

typedef struct bigsi_hip_associate_info {
    uint32_t num_unique, min_kmers, samples_hit, grouped_hit;      /* samples_hit: every hit column; grouped_hit: those in a group */
} bigsi_hip_associate_info;

int bigsi_hip_associate_batch(bigsi_hip_batch *b, const uint32_t *group_of, uint64_t n_entries, uint32_t n_groups,
                              uint32_t *counts, bigsi_hip_associate_info *info, uint64_t capacity /* sequences */);
int bigsi_hip_associate_stream(bigsi_hip_index *ix, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold,
                               const uint32_t *group_of, uint64_t n_entries, uint32_t n_groups, uint32_t *counts, bigsi_hip_associate_info *info);

#ifdef __cplusplus
}
#endif

#endif /* BIGSI_HIP_ASSOCIATE_H */
