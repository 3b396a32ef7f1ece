/*
 * bigsi_hip_prevalence.h -- k-mer prevalence of libbigsi_hip.so: for every k-mer position of a query, how many samples hold it.
 *
 * Part of the QUERY layer of the C ABI (include/bigsi_hip.h): entry points in that header's conventions (return codes,
 * bigsi_hip_last_error, one thread per handle, the row format).  A header of its own because bigsi_hip.h is kept to 60 entry points
 * (tests/test_abi_and_host.py pins it): the Python binding lists these in PREVALENCE_SIGNATURES.
 */
#ifndef BIGSI_HIP_PREVALENCE_H
#define BIGSI_HIP_PREVALENCE_H

#include "bigsi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* K-mer prevalence: the transposed question of a search.  Sequence i of a batch has n_i = max(len_i - k + 1, 0) k-mer positions;
 * for position p let A_p be the AND of the h rows of the k-mer at p (canonicalised and hashed as a search does), V the columns
 * < num_cols, U the `universe` mask (all ones when NULL) and S the `subset` mask.  Then
 *     total[pos_offsets[i] + p]     = popcount(A_p & V & U)
 *     in_subset[pos_offsets[i] + p] = popcount(A_p & V & U & S)        (only when a subset is given)
 * Positions that carry the same k-mer carry the same numbers: a k-mer is swept once on the device (one pass over its rows, the
 * popcount alone leaves the device) and the numbers are expanded over the positions, as the presence strings are.  Masks are bit
 * vectors in the row format, row_bytes bytes as bigsi_hip_get_rows writes a row; their bits at columns >= num_cols are ignored, and
 * bits that bigsi_hip_set_rows put into the matrix at columns >= num_cols are never counted.
 *   kmer_prevalence        one call, host sequences in, host counts out (the arguments of bigsi_hip_search_batch).  pos_offsets
 *                          gets n_seqs + 1 entries; `capacity` is the number of entries of total (and of in_subset).
 *                          BIGSI_ERR_CAPACITY when capacity < pos_offsets[n_seqs]: pos_offsets is filled, total / in_subset are
 *                          untouched.  The sequences are run as an exact search in a workspace of the index (the row-AND on top of
 *                          the sweep is what leaves the k-mers' row ids behind on every route), so an index without columns gets
 *                          BIGSI_ERR_STATE as a search does.
 *                          The workspace is created at the first call and lives until bigsi_hip_close, like
 *                          bigsi_hip_search_batch's: it keeps the device arrays its last call needed (a few hundred MB after
 *                          8192 x 1 kbp queries), so a caller in a loop allocates once.
 *   batch_kmer_prevalence  the same for a batch that has completed a run of any kind (BIGSI_ERR_STATE otherwise, as
 *                          bigsi_hip_batch_lookup): positions in batch order, sequence i from its pos_offset on (the prefix sums of
 *                          bigsi_hip_batch_fetch_unique's num_kmers); BIGSI_ERR_CAPACITY when capacity is below their number.
 *                          A batch of explicit k-mers (bigsi_hip_batch_create_elements) is out of scope: BIGSI_ERR_STATE.
 * BIGSI_ERR_INVALID: a NULL total or pos_offsets, in_subset without subset or subset without in_subset, and what a batch's
 * arguments are refused for (NULL pointers, n_seqs == 0, k == 0, descending offsets).  Both calls only read the index: ipc and
 * view handles are fine.  There are no group twins: the prevalence over a device group is this sweep per column shard plus a host
 * sum, a follow-up that has had no multi-GPU hardware to run on. */
int bigsi_hip_kmer_prevalence(bigsi_hip_index *ix, const char *seqs, const uint64_t *offsets, uint32_t n_seqs, uint32_t k,
                              const uint8_t *universe /* row_bytes or NULL */, const uint8_t *subset /* row_bytes or NULL */,
                              uint64_t *pos_offsets /* n_seqs + 1 */, uint32_t *total, uint32_t *in_subset /* NULL iff subset is NULL */,
                              uint64_t capacity /* entries of total / in_subset */);
int bigsi_hip_batch_kmer_prevalence(bigsi_hip_batch *b, const uint8_t *universe, const uint8_t *subset,
                                    uint32_t *total, uint32_t *in_subset, uint64_t capacity);

#ifdef __cplusplus
}
#endif

#endif /* BIGSI_HIP_PREVALENCE_H */
