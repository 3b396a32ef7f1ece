/*
 * bigsi_hip_compact.h -- column compaction of libbigsi_hip.so: remove or extract samples PHYSICALLY.
 *
 * The MAINTENANCE layer of the C ABI (include/bigsi_hip.h), part of CORE in meaning: single-index entry points in that header's
 * conventions (return codes, bigsi_hip_last_error, one thread per handle, the row format).  A header of its own because a host
 * that only serves queries never needs it, and because bigsi_hip.h is kept to 60 entry points (tests/test_abi_and_host.py pins that
 * number, and the Python binding's SIGNATURES table to the four earlier headers): the binding lists these in COMPACT_SIGNATURES.
 */
#ifndef BIGSI_HIP_COMPACT_H
#define BIGSI_HIP_COMPACT_H

#include "bigsi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Column compaction: remove or extract samples physically (no counterpart in the reference: its delete_sample only renames the
 * colour, bigsi/graph/metadata.py, and the column stays in every row for good).  keep: ceil(num_cols/8) bytes in the row format --
 * column c at byte c/8 under mask 0x80 >> (c%8); bits at columns >= num_cols are ignored.  With K = popcount(keep), the j-th kept
 * column of every row becomes column j, in the old order, and every bit from column K to the end of the row stride is zero
 * afterwards.  All bits kept is valid (the matrix stays byte-identical); no bits kept is valid (num_cols 0, every row zero).
 * A NULL index or keep: BIGSI_ERR_INVALID.
 *   compact_columns  in place: num_cols becomes K, stride and capacity stay (bigsi_hip_shrink_to_fit gives the memory back);
 *                    *new_num_cols = K (may be NULL).  A writer: ipc / view handles get BIGSI_ERR_STATE, and so does an owner
 *                    while views of it are open (their column count would go stale), as for bigsi_hip_reserve_cols.
 *   extract_columns  out of place: the kept columns of src become columns [0, K) of dst; src is only read and may be a view or
 *                    an ipc handle.  dst != src, same num_rows, same device (BIGSI_ERR_INVALID otherwise); dst must be writable
 *                    and hold no columns (num_cols == 0; BIGSI_ERR_STATE otherwise); its capacity grows as needed.  While views
 *                    of dst are open the call is refused as well (BIGSI_ERR_STATE: their column count would go stale).  Both
 *                    handles are held for the duration of the call (one thread per handle): BIGSI_ERR_STATE when another
 *                    host thread is inside src.
 *   shrink_to_fit    re-stride DOWN to the stride of max(num_cols, 1) columns: the counterpart of bigsi_hip_reserve_cols, which
 *                    only grows.  A no-op when the stride is already minimal; otherwise a writer that moves the matrix:
 *                    BIGSI_ERR_STATE for ipc / view handles and while views are open.  Needs room for the smaller copy beside
 *                    the matrix while it runs.
 * Batches of the index stay valid, as across bigsi_hip_set_num_cols / bigsi_hip_insert_columns: every run takes the column count
 * the index has at that moment, so runs after the call see the new colours; results of a run made BEFORE the call carry the old
 * colour numbers and must be fetched (or dropped) first, and a limit's excluded colours (bigsi_hip_batch_set_limit) are the
 * caller's to renumber.  There are no group twins: column shards have a fixed width, and moving columns across shards is another
 * operation. */
int bigsi_hip_compact_columns(bigsi_hip_index *ix, const uint8_t *keep, uint64_t *new_num_cols);
int bigsi_hip_extract_columns(bigsi_hip_index *dst, const bigsi_hip_index *src, const uint8_t *keep);
int bigsi_hip_shrink_to_fit(bigsi_hip_index *ix);

#ifdef __cplusplus
}
#endif

#endif /* BIGSI_HIP_COMPACT_H */
