/*
 * bigsi_cpu_consensus.h -- libbigsi_cpu.so: the CPU twin of include/bigsi_hip_consensus.h (consensus collapse), as bigsi_cpu.h is the
 * twin of the CORE layer of bigsi_hip.h: same entry point, same argument meaning, same error codes, same row format, same results --
 * computed on the host one row and one column at a time.  Shares no code with the device path.
 */
#ifndef BIGSI_CPU_CONSENSUS_H
#define BIGSI_CPU_CONSENSUS_H

#include "bigsi_cpu.h"
#include "bigsi_hip_consensus.h"

#ifdef __cplusplus
extern "C" {
#endif

int bigsi_cpu_consensus_columns_into(bigsi_cpu_index *dst, const bigsi_cpu_index *src, const uint32_t *group_of, uint64_t num_groups,
                                     const uint32_t *min_members);

#ifdef __cplusplus
}
#endif

/* as in bigsi_cpu.h: a host written against bigsi_hip_consensus.h, built against the twin */
#ifdef BIGSI_USE_CPU_TWIN
#define bigsi_hip_consensus_columns_into bigsi_cpu_consensus_columns_into
#endif

#endif /* BIGSI_CPU_CONSENSUS_H */
