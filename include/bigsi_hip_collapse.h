/*
 * bigsi_hip_collapse.h -- column collapse of libbigsi_hip.so: OR the columns of a group of samples into one column of a new index.
 *
 * The MAINTENANCE layer of the C ABI (include/bigsi_hip.h), beside include/bigsi_hip_compact.h (remove or select columns) and
 * include/bigsi_hip_fold.h (OR rows): single-index entry points in bigsi_hip.h's conventions (return codes, bigsi_hip_last_error, one
 * thread per handle, the row format).  A header of its own for the reason bigsi_hip_compact.h gives: bigsi_hip.h is kept to 60 entry
 * points; the binding lists this one in COLLAPSE_SIGNATURES.
 */
#ifndef BIGSI_HIP_COLLAPSE_H
#define BIGSI_HIP_COLLAPSE_H

#include "bigsi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* group_of[c] of a dropped source column */
#define BIGSI_COLLAPSE_DROPPED 0xFFFFFFFFu

/* Column collapse (no counterpart in the reference).  group_of: src.num_cols entries, each a group id in [0, num_groups) or
 * BIGSI_COLLAPSE_DROPPED.  Destination column g of every row becomes the OR of the source columns c with group_of[c] == g: the Bloom
 * filter of a union of k-mer sets is the OR of the members' filters, so dst is bit for bit the index built from the OR-ed filters,
 * and a hit of any member is a hit of its group (no false negatives).  A group without members gives a zero column; an injective map
 * reorders samples.  dst.num_cols becomes num_groups; the whole destination stride is written, every bit from column num_groups to
 * its end is zero, and source bits at columns >= src.num_cols never survive.  src is only read and may be a view or an ipc handle.
 * dst's capacity grows as needed (as for bigsi_hip_extract_columns).  The call holds both handles for its duration (one thread per
 * handle: BIGSI_ERR_STATE if another thread is inside either).
 *   BIGSI_ERR_INVALID  a NULL argument; num_groups == 0 or >= 2^32 - 1; an entry >= num_groups that is not BIGSI_COLLAPSE_DROPPED
 *                      (the message names the column and the value); dst == src, or one a view of the other's matrix; another
 *                      device; another num_rows; another num_hashes.
 *   BIGSI_ERR_STATE    dst holds columns (num_cols != 0); dst is read-only (ipc / view); dst is an owner with views open.
 * A refused call leaves dst as it was.  There is no in-place form (a many-to-one map has no safe in-place order, and the use is a
 * new index) and there are no group twins, as for compaction. */
int bigsi_hip_collapse_columns_into(bigsi_hip_index *dst, const bigsi_hip_index *src, const uint32_t *group_of, uint64_t num_groups);

#ifdef __cplusplus
}
#endif

#endif /* BIGSI_HIP_COLLAPSE_H */
