/*
 * bigsi_cpu_typing.h -- libbigsi_cpu.so: the CPU twin of include/bigsi_hip_typing.h (locus typing), as bigsi_cpu.h is the twin of
 * the CORE layer of bigsi_hip.h: same meaning, same error codes, same outputs -- computed on the host, record by record in the
 * reference's shape (the search of bigsi_cpu_search_batch, a loop over its hit columns).  Shares no code with the device path: the
 * key is written out in the twin on its own.  The twin has no accumulator and no batch objects: ONE call takes the whole set.
 */
#ifndef BIGSI_CPU_TYPING_H
#define BIGSI_CPU_TYPING_H

#include "bigsi_cpu.h"
#include "bigsi_hip_typing.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The outputs of bigsi_hip_typing_fetch behind one bigsi_hip_typing_add_stream of the whole set: best (uint64) / hits (uint32),
 * n_loci rows of num_cols entries (either may be NULL), locus_counts n_loci x 3, sample_counts num_cols x 2, records n_loci.
 * BIGSI_ERR_INVALID: a NULL argument, n_seqs == 0, k == 0, descending offsets, a threshold above 1, n_loci outside 1 ..
 * BIGSI_TYPING_MAX_LOCI, a locus_of value that is neither below n_loci nor BIGSI_TYPING_NONE, an allele_of value above
 * BIGSI_TYPING_MAX_ALLELE (of a record with a locus); BIGSI_ERR_STATE: an index without columns; BIGSI_ERR_NOMEM: cells above
 * BIGSI_TYPING_CELL_BYTES; BIGSI_ERR_CAPACITY as the fetch.  A refused call writes nothing. */
int bigsi_cpu_typing(bigsi_cpu_index *ix, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold,
                     const uint32_t *locus_of, const uint32_t *allele_of, uint32_t n_loci, const uint8_t *columns /* or NULL */, uint64_t *best /* or NULL */,
                     uint32_t *hits /* or NULL */, uint64_t cell_capacity, uint32_t *locus_counts, uint32_t *sample_counts, uint64_t sample_capacity,
                     uint32_t *records);

#ifdef __cplusplus
}
#endif

#endif /* BIGSI_CPU_TYPING_H */
