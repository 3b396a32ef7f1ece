/*
 * bigsi_cpu_classify.h -- libbigsi_cpu.so: the CPU twin of include/bigsi_hip_classify.h (read classification), as bigsi_cpu.h is the
 * twin of the CORE layer of bigsi_hip.h: same meaning, same error codes, same row format, same records -- computed on the host,
 * sequence by sequence in the reference's shape (the search of bigsi_cpu_search_batch, its hits weighed per group).  Shares no code
 * with the device path.  The twin has no batch objects: ONE call takes the whole set and writes one record per sequence.
 */
#ifndef BIGSI_CPU_CLASSIFY_H
#define BIGSI_CPU_CLASSIFY_H

#include "bigsi_cpu.h"
#include "bigsi_hip_classify.h"

#ifdef __cplusplus
extern "C" {
#endif

/* records: n_seqs entries, as bigsi_hip_classify_stream writes them.  BIGSI_ERR_INVALID: a NULL argument, n_seqs == 0, k == 0,
 * descending offsets, a threshold above 1, n_entries != num_cols, n_groups outside 1 .. BIGSI_CLASSIFY_MAX_GROUPS, a group_of value
 * that is neither below n_groups nor BIGSI_CLASSIFY_NONE; BIGSI_ERR_STATE: an index without columns.  A refused call writes nothing. */
int bigsi_cpu_classify(bigsi_cpu_index *ix, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold,
                       const uint32_t *group_of, uint64_t n_entries, uint32_t n_groups, bigsi_hip_classify_record *records);

#ifdef __cplusplus
}
#endif

#endif /* BIGSI_CPU_CLASSIFY_H */
