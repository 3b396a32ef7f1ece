/*
 * bigsi_cpu_compact.h -- libbigsi_cpu.so: the CPU twin of include/bigsi_hip_compact.h (column compaction), as bigsi_cpu.h is the
 * twin of the CORE layer of bigsi_hip.h: same entry points, same argument meaning, same error codes, same row format, same
 * results -- computed on the host one row and one column at a time.  Shares no code with the device path.
 * bigsi_hip_shrink_to_fit has no twin: the twin's row stride is host bookkeeping that no result depends on (the device's is HBM
 * that a vacuum wants back).
 */
#ifndef BIGSI_CPU_COMPACT_H
#define BIGSI_CPU_COMPACT_H

#include "bigsi_cpu.h"
#include "bigsi_hip_compact.h"

#ifdef __cplusplus
extern "C" {
#endif

int bigsi_cpu_compact_columns(bigsi_cpu_index *ix, const uint8_t *keep, uint64_t *new_num_cols);
int bigsi_cpu_extract_columns(bigsi_cpu_index *dst, const bigsi_cpu_index *src, const uint8_t *keep);

#ifdef __cplusplus
}
#endif

/* as in bigsi_cpu.h: a host written against bigsi_hip_compact.h, built against the twin */
#ifdef BIGSI_USE_CPU_TWIN
#define bigsi_hip_compact_columns bigsi_cpu_compact_columns
#define bigsi_hip_extract_columns bigsi_cpu_extract_columns
#endif

#endif /* BIGSI_CPU_COMPACT_H */
