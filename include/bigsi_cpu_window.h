/*
 * bigsi_cpu_window.h -- libbigsi_cpu.so: the CPU twin of include/bigsi_hip_window.h (windowed search), as bigsi_cpu.h is the twin of
 * the CORE layer of bigsi_hip.h: same arguments, same meaning, same error codes, same row format, same results -- computed on the
 * host as a plain loop over positions with a prefix sum per column.  Shares no code with the device path.  The twin has no batch
 * objects, so there is no twin of bigsi_hip_batch_window_search.
 */
#ifndef BIGSI_CPU_WINDOW_H
#define BIGSI_CPU_WINDOW_H

#include "bigsi_cpu.h"
#include "bigsi_hip_window.h"

#ifdef __cplusplus
extern "C" {
#endif

int bigsi_cpu_window_search(bigsi_cpu_index *ix, const char *seqs, const uint64_t *offsets, uint32_t n_seqs, uint32_t k,
                            uint32_t window, double threshold, uint32_t *window_used /* n_seqs */, uint32_t *need /* n_seqs */,
                            uint64_t *hit_offsets /* n_seqs + 1 */, uint32_t *colours, bigsi_hip_window_hit *records,
                            uint64_t capacity /* entries of colours / records */);

#ifdef __cplusplus
}
#endif

/* as in bigsi_cpu.h: a host written against bigsi_hip_window.h, built against the twin */
#ifdef BIGSI_USE_CPU_TWIN
#define bigsi_hip_window_search bigsi_cpu_window_search
#endif

#endif /* BIGSI_CPU_WINDOW_H */
