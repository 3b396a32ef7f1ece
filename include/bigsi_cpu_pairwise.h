/*
 * bigsi_cpu_pairwise.h -- libbigsi_cpu.so: the CPU twin of include/bigsi_hip_pairwise.h (pairwise popcounts), as bigsi_cpu.h is the
 * twin of the CORE layer of bigsi_hip.h: same entry point, same argument meaning, same checks in the same order, same error codes,
 * same results -- computed on the host one row and one pair at a time (nothing is transposed).  Shares no code with the device path.
 */
#ifndef BIGSI_CPU_PAIRWISE_H
#define BIGSI_CPU_PAIRWISE_H

#include "bigsi_cpu.h"
#include "bigsi_hip_pairwise.h"

#ifdef __cplusplus
extern "C" {
#endif

int bigsi_cpu_pairwise_popcounts(bigsi_cpu_index *ix, const uint32_t *cols_a, uint64_t na, const uint32_t *cols_b, uint64_t nb, uint64_t *out,
                                 uint64_t capacity);

#ifdef __cplusplus
}
#endif

/* as in bigsi_cpu.h: a host written against bigsi_hip_pairwise.h, built against the twin */
#ifdef BIGSI_USE_CPU_TWIN
#define bigsi_hip_pairwise_popcounts bigsi_cpu_pairwise_popcounts
#endif

#endif /* BIGSI_CPU_PAIRWISE_H */
