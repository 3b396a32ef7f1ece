/*
 * bigsi_cpu_fold.h -- libbigsi_cpu.so: the CPU twin of include/bigsi_hip_fold.h (row folding), as bigsi_cpu.h is the twin of the
 * CORE layer of bigsi_hip.h: same entry points, same argument meaning, same error codes, same row format, same results --
 * computed on the host as plain loops over rows and bytes.  Shares no code with the device path.  The twin's trim_rows really
 * reallocates.
 */
#ifndef BIGSI_CPU_FOLD_H
#define BIGSI_CPU_FOLD_H

#include "bigsi_cpu.h"
#include "bigsi_hip_fold.h"

#ifdef __cplusplus
extern "C" {
#endif

int bigsi_cpu_fold_rows(bigsi_cpu_index *ix, uint64_t factor, uint64_t *new_num_rows);
int bigsi_cpu_fold_rows_into(bigsi_cpu_index *dst, const bigsi_cpu_index *src);
int bigsi_cpu_trim_rows(bigsi_cpu_index *ix);

#ifdef __cplusplus
}
#endif

/* as in bigsi_cpu.h: a host written against bigsi_hip_fold.h, built against the twin */
#ifdef BIGSI_USE_CPU_TWIN
#define bigsi_hip_fold_rows bigsi_cpu_fold_rows
#define bigsi_hip_fold_rows_into bigsi_cpu_fold_rows_into
#define bigsi_hip_trim_rows bigsi_cpu_trim_rows
#endif

#endif /* BIGSI_CPU_FOLD_H */
