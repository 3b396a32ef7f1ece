/*
 * bigsi_hip_genotype.h -- panel genotyping of libbigsi_hip.so: for a panel of variants, each with probes that carry its reference
 * allele and probes that carry its alternate allele, every sample's call (0/0, 0/1, 1/1 or missing) -- the probes' result vectors
 * ORed into one bit plane per allele on the device, the calls taken from two planes by AND, AND-NOT and popcount.  No hit list is
 * built: 2 bits per (variant, sample), four counts per variant and two per sample leave the device.
 *
 * Part of the QUERY layer of the C ABI (include/bigsi_hip.h): entry points in that header's conventions (return codes,
 * bigsi_hip_last_error, one thread per handle, the row format).  A header of its own because bigsi_hip.h is kept to 60 entry points
 * (tests/test_abi_and_host.py pins it): the Python binding lists these in GENOTYPE_SIGNATURES.
 */
#ifndef BIGSI_HIP_GENOTYPE_H
#define BIGSI_HIP_GENOTYPE_H

#include "bigsi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What is computed.  Inputs: probes (sequences), k, a threshold t <= 1; allele_of[n_seqs] (uint32: 2 v + a with v < n_variants and
 * a = 0 for a ref probe, 1 for an alt probe, or BIGSI_GENOTYPE_NONE: the probe is ignored); an optional column selection `columns`, a
 * bit vector in the row format of ceil(num_cols / 8) bytes (NULL: every column; bits behind num_cols are ignored).  For probe i the
 * quantities are those of bigsi_hip_tally.h: u_i its distinct k-mers and hit_i[s], s < num_cols, the hit bigsi_hip_search_batch
 * reports at threshold t.  A probe with u_i > 0 and an allele 2 v + a does
 *     plane[v][a][s] |= hit_i[s]        for selected s
 *     used[v][a]     += 1               (uint32)
 * and a probe with u_i == 0 or BIGSI_GENOTYPE_NONE changes nothing.  For a selected column s, with r = plane[v][0][s] and
 * a = plane[v][1][s], the call is 0/0 (r and not a), 0/1 (r and a), 1/1 (a and not r) or missing (neither) -- genotypes() of
 * bigsi_amd/variant_search.py.  Out come
 *     ref_planes, alt_planes   n_variants rows of ceil(num_cols / 8) bytes each, row format; unselected and pad bits zero
 *     variant_counts[v]        { hom_ref, het, hom_alt, missing }, 4 x uint32 over the selected columns
 *     sample_counts[s]         { carried, called }, 2 x uint32 for s < num_cols: the variants with a set; those with r | a set.  An
 *                              unselected column gets zeros
 *     allele_probes[v]         { used[v][0], used[v][1] }
 * Everything is integer OR / AND / popcount / add: bit-identical under any order of the probes, any cut into batches or chunks, and
 * from run to run.
 *
 * Limits.  n_variants is at most BIGSI_GENOTYPE_MAX_VARIANTS, and both planes of all variants -- 2 x n_variants x ceil(num_cols / 64)
 * x 8 bytes of device memory, held for the accumulator's life -- at most BIGSI_GENOTYPE_PLANE_BYTES.  4 GiB is a DESIGN limit, not a
 * measured one: it is 17179 variants at a million samples, and a caller with a larger panel slices it by variant (every slice an
 * accumulator of its own, a probe going to its variant's slice only), as bigsi_amd's BIGSI.genotype_arrays does.
 *
 *   genotype_create     device planes and counts, zeroed, for the index's num_cols at this moment and the selection.  The accumulator
 *                       belongs to the index: destroy it before bigsi_hip_close.  An index whose num_cols, num_rows or num_hashes
 *                       have changed since gets BIGSI_ERR_STATE from every call but destroy.
 *   genotype_reset      zeroes planes and used (and makes an accumulator usable again after a failed genotype_add_stream).
 *   genotype_add_batch  adds a batch of this index whose last run was made with BIGSI_RUN_SKIP_COMPACT (exact or counting, dense or
 *                       BIGSI_RUN_SPARSE_COUNTS: no counter is read).  allele_of (n_entries == the batch's n_seqs) is validated on
 *                       the host first -- a bad value is BIGSI_ERR_INVALID naming the probe, and nothing is added -- then uploaded,
 *                       and k_allele_or is queued on the stream the run finished on.  The batch's completion event is recorded again
 *                       behind it, so bigsi_hip_batch_reload, bigsi_hip_batch_run and bigsi_hip_batch_destroy directly afterwards
 *                       are safe without any synchronisation by the caller, and allele_of is no longer read when the call returns.
 *                       BIGSI_ERR_STATE for a batch of another index and for what bigsi_hip_tally_add_batch refuses a batch for.
 *   genotype_add_stream any number of host sequences (the arguments of bigsi_hip_search_stream) and their allele_of[n_seqs]: cut
 *                       into device batches by the tally's rule (include/bigsi_hip_tally.h) that alternate over two workspaces of
 *                       the index of the call's own.  A chunk without a k-mer position adds nothing.  On a failure the workspaces
 *                       are destroyed and the accumulator is marked unusable (every call but reset and destroy: BIGSI_ERR_STATE).
 *   genotype_fetch      waits for everything added so far, computes the calls from the planes (every time: a second fetch returns
 *                       the same; the planes keep accumulating afterwards) and copies out.  ref_planes / alt_planes may be NULL:
 *                       that plane is not copied.  BIGSI_ERR_CAPACITY when plane_capacity_bytes < n_variants x ceil(num_cols / 8)
 *                       (with a plane asked for) or sample_capacity < num_cols: nothing is written.
 * BIGSI_ERR_INVALID: a NULL argument, n_variants == 0 or above BIGSI_GENOTYPE_MAX_VARIANTS, n_entries != n_seqs, an allele_of value
 * that is neither below 2 n_variants nor BIGSI_GENOTYPE_NONE, and what a stream's arguments are refused for.  BIGSI_ERR_NOMEM: planes
 * above BIGSI_GENOTYPE_PLANE_BYTES.  BIGSI_ERR_STATE: an index without columns.  All calls only read the index: ipc and view handles
 * are fine.  There are no group twins. */
#define BIGSI_GENOTYPE_NONE 0xFFFFFFFFu
#define BIGSI_GENOTYPE_MAX_VARIANTS (1u << 20)
#define BIGSI_GENOTYPE_PLANE_BYTES (4ull << 30)

typedef struct bigsi_hip_genotype bigsi_hip_genotype;
int bigsi_hip_genotype_create(bigsi_hip_index *ix, uint32_t n_variants, const uint8_t *columns /* or NULL */, bigsi_hip_genotype **out);
int bigsi_hip_genotype_destroy(bigsi_hip_genotype *g);
int bigsi_hip_genotype_reset(bigsi_hip_genotype *g);
int bigsi_hip_genotype_add_batch(bigsi_hip_genotype *g, bigsi_hip_batch *b, const uint32_t *allele_of, uint64_t n_entries);
int bigsi_hip_genotype_add_stream(bigsi_hip_genotype *g, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold,
                                  const uint32_t *allele_of);
int bigsi_hip_genotype_fetch(bigsi_hip_genotype *g, uint8_t *ref_planes, uint8_t *alt_planes, uint64_t plane_capacity_bytes,
                             uint32_t *variant_counts, uint32_t *sample_counts, uint64_t sample_capacity, uint32_t *allele_probes);

#ifdef __cplusplus
}
#endif

#endif /* BIGSI_HIP_GENOTYPE_H */
