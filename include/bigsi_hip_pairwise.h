/*
 * bigsi_hip_pairwise.h -- pairwise sample overlap of libbigsi_hip.so: the shared-bit counts of every pair of two lists of columns.
 *
 * The STATISTICS beside bigsi_hip_column_popcounts (include/bigsi_hip.h): a single-index entry point in bigsi_hip.h's conventions
 * (return codes, bigsi_hip_last_error, one thread per handle, the row format).  A header of its own for the reason
 * bigsi_hip_compact.h gives: bigsi_hip.h is kept to 60 entry points; the binding lists this one in PAIRWISE_SIGNATURES.
 */
#ifndef BIGSI_HIP_PAIRWISE_H
#define BIGSI_HIP_PAIRWISE_H

#include "bigsi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most pairs (na x nb) of one call: 2 GiB of uint64 */
#define BIGSI_PAIRWISE_MAX_PAIRS (1ull << 28)

/* Pairwise popcounts (no counterpart in the reference): the bit-matrix product of the selected columns.
 * out[i * nb + j] = number of rows r < num_rows with bit (r, cols_a[i]) AND bit (r, cols_b[j]) set.
 * cols_b == NULL (nb ignored): cols_b = cols_a, the full square matrix is written (both triangles; the diagonal is the column's own
 * popcount, equal to bigsi_hip_column_popcounts).  The lists may be unsorted and may repeat a column; a repeated column repeats its
 * row or column of out.  Counts are exact for any num_rows; rows the allocation holds behind num_rows (after an in-place
 * bigsi_hip_fold_rows, until bigsi_hip_trim_rows) are never counted.  The index is only read: view and ipc handles are served; the
 * call holds the handle for its duration (one thread per handle).  One pass over the selected columns' words, then VALU work in
 * proportion to na x nb x num_rows / 64; device scratch does not grow with num_rows (the rows are taken in chunks) and lives for
 * this call only, beside 8 bytes per pair for the result.  The arguments are checked in this order, before the handle's state:
 *   BIGSI_ERR_INVALID   a NULL index, cols_a or out; na == 0; cols_b != NULL and nb == 0.
 *   BIGSI_ERR_RANGE     an entry >= num_cols (the message names the list, the position and the value).
 *   BIGSI_ERR_CAPACITY  capacity (entries of out) below na x nb.
 *   BIGSI_ERR_RANGE     na x nb above BIGSI_PAIRWISE_MAX_PAIRS.
 * then BIGSI_ERR_NOMEM when the scratch or the device result does not fit beside the index (nothing is leaked, no HIP error stays
 * behind).  A refused or failed call leaves out untouched.  There is no group twin. */
int bigsi_hip_pairwise_popcounts(bigsi_hip_index *ix, const uint32_t *cols_a, uint64_t na, const uint32_t *cols_b, uint64_t nb, uint64_t *out,
                                 uint64_t capacity);

/* MEASUREMENT: the kernel times of this handle's last bigsi_hip_pairwise_popcounts that ran with profiling on
 * (bigsi_hip_set_profiling level >= 1), in milliseconds, summed over the chunks: ms[0] k_columns_to_planes, ms[1] k_pair_popcount,
 * ms[2] k_pair_popcount_sum; ms[3] the chunks.  All 0 before such a call.  (With profiling on the call waits after every launch.) */
int bigsi_hip_pairwise_phase_ms(bigsi_hip_index *ix, double ms[4]);

#ifdef __cplusplus
}
#endif

#endif /* BIGSI_HIP_PAIRWISE_H */
