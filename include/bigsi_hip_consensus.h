/*
 * bigsi_hip_consensus.h -- consensus collapse of libbigsi_hip.so: one column per group of samples that keeps a bit only where at least
 * a given number of the group's members have it (the CORE of the group; include/bigsi_hip_collapse.h keeps the UNION).
 *
 * The MAINTENANCE layer of the C ABI (include/bigsi_hip.h), beside include/bigsi_hip_collapse.h: a single-index entry point in
 * bigsi_hip.h's conventions (return codes, bigsi_hip_last_error, one thread per handle, the row format).  A header of its own for the
 * reason bigsi_hip_compact.h gives: bigsi_hip.h is kept to 60 entry points, and bigsi_hip_collapse.h to its one; the binding lists
 * this one in CONSENSUS_SIGNATURES.
 */
#ifndef BIGSI_HIP_CONSENSUS_H
#define BIGSI_HIP_CONSENSUS_H

#include "bigsi_hip_collapse.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Consensus collapse (no counterpart in the reference).  group_of: exactly as for the collapse -- src.num_cols entries, each a group
 * id in [0, num_groups) or BIGSI_COLLAPSE_DROPPED.  min_members: num_groups entries, each at least 1.  Destination column g of every
 * row becomes 1 iff at least min_members[g] source columns c with group_of[c] == g are set in that row.  A k-mer held by at least
 * min_members[g] members has each of its num_hashes bits set in at least that many member columns, so all of them survive and the
 * k-mer is still found in column g (no false negatives for the k-mers of the core), while the column's fill, and with it the
 * false-positive rate, falls as min_members rises.  min_members[g] == 1 is the collapse's OR, min_members[g] == the group's size the
 * AND.  A min_members[g] larger than the group's size is legal and gives a zero column; so does a group without members.
 * dst.num_cols becomes num_groups; the whole destination stride is written, every bit from column num_groups to its end is zero, and
 * source bits at columns >= src.num_cols never count.  src is only read and may be a view or an ipc handle.  dst's capacity grows as
 * needed.  The call holds both handles for its duration (BIGSI_ERR_STATE if another thread is inside either).
 * Checks and codes are the collapse's, in its order, and after them:
 *   BIGSI_ERR_INVALID  min_members == NULL (with the other NULL arguments); min_members[g] == 0 (after the entries of group_of; the
 *                      message names g): every row would have "at least 0 members", an all-ones column.
 * A refused call leaves dst as it was.  There is no in-place form and there are no group twins, as for the collapse. */
int bigsi_hip_consensus_columns_into(bigsi_hip_index *dst, const bigsi_hip_index *src, const uint32_t *group_of, uint64_t num_groups,
                                     const uint32_t *min_members);

#ifdef __cplusplus
}
#endif

#endif /* BIGSI_HIP_CONSENSUS_H */
