/*
 * bigsi_cpu_genotype.h -- libbigsi_cpu.so: the CPU twin of include/bigsi_hip_genotype.h (panel genotyping), as bigsi_cpu.h is the
 * twin of the CORE layer of bigsi_hip.h: same meaning, same error codes, same row format, same outputs -- computed on the host,
 * probe by probe in the reference's shape (the search of bigsi_cpu_search_batch, a loop over its hit columns).  Shares no code with
 * the device path.  The twin has no accumulator and no batch objects: ONE call takes the whole set.
 */
#ifndef BIGSI_CPU_GENOTYPE_H
#define BIGSI_CPU_GENOTYPE_H

#include "bigsi_cpu.h"
#include "bigsi_hip_genotype.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The outputs of bigsi_hip_genotype_fetch behind one bigsi_hip_genotype_add_stream of the whole set: ref_planes / alt_planes (either
 * may be NULL) n_variants rows of ceil(num_cols / 8) bytes, variant_counts n_variants x 4, sample_counts num_cols x 2, allele_probes
 * n_variants x 2.  BIGSI_ERR_INVALID: a NULL argument, n_seqs == 0, k == 0, descending offsets, a threshold above 1, n_variants
 * outside 1 .. BIGSI_GENOTYPE_MAX_VARIANTS, an allele_of value that is neither below 2 n_variants nor BIGSI_GENOTYPE_NONE;
 * BIGSI_ERR_STATE: an index without columns; BIGSI_ERR_NOMEM: planes above BIGSI_GENOTYPE_PLANE_BYTES; BIGSI_ERR_CAPACITY as the
 * fetch.  A refused call writes nothing. */
int bigsi_cpu_genotype(bigsi_cpu_index *ix, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold,
                       const uint32_t *allele_of, uint32_t n_variants, const uint8_t *columns /* or NULL */, uint8_t *ref_planes, uint8_t *alt_planes,
                       uint64_t plane_capacity_bytes, uint32_t *variant_counts, uint32_t *sample_counts, uint64_t sample_capacity, uint32_t *allele_probes);

#ifdef __cplusplus
}
#endif

#endif /* BIGSI_CPU_GENOTYPE_H */
