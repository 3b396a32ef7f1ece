/*
 * bigsi_cpu_associate.h -- libbigsi_cpu.so: the CPU twin of include/bigsi_hip_associate.h (group association), as bigsi_cpu.h is the
 * twin of the CORE layer of bigsi_hip.h: same meaning, same error codes, same row format, same outputs -- computed on the host,
 * sequence by sequence in the reference's shape (the search of bigsi_cpu_search_batch, a loop over its hit columns).  Shares no code
 * with the device path.  The twin has no batch objects: ONE call takes the whole set.
 */
#ifndef BIGSI_CPU_ASSOCIATE_H
#define BIGSI_CPU_ASSOCIATE_H

#include "bigsi_cpu.h"
#include "bigsi_hip_associate.h"

#ifdef __cplusplus
extern "C" {
#endif

/* counts: n_seqs x n_groups entries, info: n_seqs, as bigsi_hip_associate_stream writes them.  BIGSI_ERR_INVALID: a NULL argument,
 * n_seqs == 0, k == 0, descending offsets, a threshold above 1, n_entries != num_cols, n_groups outside 1 ..
 * BIGSI_ASSOCIATE_MAX_GROUPS, a group_of value that is neither below n_groups nor BIGSI_ASSOCIATE_NONE; BIGSI_ERR_STATE: an index
 * without columns.  A refused call writes nothing. */
int bigsi_cpu_associate(bigsi_cpu_index *ix, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold,
                        const uint32_t *group_of, uint64_t n_entries, uint32_t n_groups, uint32_t *counts, bigsi_hip_associate_info *info);

#ifdef __cplusplus
}
#endif

#endif /* BIGSI_CPU_ASSOCIATE_H */
