/*
 * bigsi_cpu_prevalence.h -- libbigsi_cpu.so: the CPU twin of include/bigsi_hip_prevalence.h (k-mer prevalence), as bigsi_cpu.h is
 * the twin of the CORE layer of bigsi_hip.h: same arguments, same meaning, same error codes, same row format, same results --
 * computed on the host as plain loops over k-mers, rows and bytes.  Shares no code with the device path.  The twin has no batch
 * objects, so there is no twin of bigsi_hip_batch_kmer_prevalence.
 */
#ifndef BIGSI_CPU_PREVALENCE_H
#define BIGSI_CPU_PREVALENCE_H

#include "bigsi_cpu.h"
#include "bigsi_hip_prevalence.h"

#ifdef __cplusplus
extern "C" {
#endif

int bigsi_cpu_kmer_prevalence(bigsi_cpu_index *ix, const char *seqs, const uint64_t *offsets, uint32_t n_seqs, uint32_t k,
                              const uint8_t *universe /* row_bytes or NULL */, const uint8_t *subset /* row_bytes or NULL */,
                              uint64_t *pos_offsets /* n_seqs + 1 */, uint32_t *total, uint32_t *in_subset /* NULL iff subset is NULL */,
                              uint64_t capacity /* entries of total / in_subset */);

#ifdef __cplusplus
}
#endif

/* as in bigsi_cpu.h: a host written against bigsi_hip_prevalence.h, built against the twin */
#ifdef BIGSI_USE_CPU_TWIN
#define bigsi_hip_kmer_prevalence bigsi_cpu_kmer_prevalence
#endif

#endif /* BIGSI_CPU_PREVALENCE_H */
