/*
 * bigsi_cpu_tally.h -- libbigsi_cpu.so: the CPU twin of include/bigsi_hip_tally.h (query-set tally), as bigsi_cpu.h is the twin of
 * the CORE layer of bigsi_hip.h: same meaning, same error codes, same row format, same results -- computed on the host, sequence by
 * sequence in the reference's shape (the search of bigsi_cpu_search_batch, its hits summed).  Shares no code with the device path.
 * The twin has no batch objects and no handle to accumulate in: ONE call takes the whole set and writes the sums.
 */
#ifndef BIGSI_CPU_TALLY_H
#define BIGSI_CPU_TALLY_H

#include "bigsi_cpu.h"
#include "bigsi_hip_tally.h"

#ifdef __cplusplus
extern "C" {
#endif

/* queries_hit / kmers_found: num_cols entries each (BIGSI_ERR_CAPACITY when capacity < num_cols: nothing is written); totals[4] as
 * bigsi_hip_tally_fetch.  BIGSI_ERR_INVALID: a NULL argument, n_seqs == 0, k == 0, descending offsets, a threshold above 1;
 * BIGSI_ERR_STATE: an index without columns. */
int bigsi_cpu_search_tally(bigsi_cpu_index *ix, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold,
                           uint64_t *queries_hit, uint64_t *kmers_found, uint64_t capacity, uint64_t totals[4]);

#ifdef __cplusplus
}
#endif

#endif /* BIGSI_CPU_TALLY_H */
