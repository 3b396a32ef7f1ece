/*
 * bigsi_hip_typing.h -- locus typing of libbigsi_hip.so: for a catalogue of allele records grouped into loci (an MLST or cgMLST
 * scheme, serotype or capsule genes, the variants of a resistance gene), which allele of each locus every sample carries -- per
 * (locus, sample) the record with the highest fraction of its k-mers found, taken on the device by a segmented max over the result
 * vectors and counters of the records.  No hit list is built: 12 bytes per (locus, sample), three counts per locus and two per
 * sample leave the device.
 *
 * Part of the QUERY layer of the C ABI (include/bigsi_hip.h): entry points in that header's conventions (return codes,
 * bigsi_hip_last_error, one thread per handle, the row format).  A header of its own because bigsi_hip.h is kept to 60 entry points
 * (tests/test_abi_and_host.py pins it): the Python binding lists these in TYPING_SIGNATURES.
 */
#ifndef BIGSI_HIP_TYPING_H
#define BIGSI_HIP_TYPING_H

#include "bigsi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What is computed.  Inputs: records (sequences), k, a threshold t <= 1; two labels per record -- locus_of[i] (uint32: a locus
 * < n_loci, or BIGSI_TYPING_NONE: the record is ignored, and its allele_of is not looked at) and allele_of[i] (uint32: an identity
 * <= BIGSI_TYPING_MAX_ALLELE; it is the caller's, global over all adds) --; an optional column selection `columns`, a bit vector in
 * the row format of ceil(num_cols / 8) bytes (NULL: every column; bits behind num_cols are ignored).  For record i the quantities
 * are those of bigsi_hip_tally.h: u_i its distinct k-mers, mk_i = ceil(u_i t) clamped at 0, c_i[s] the number of them sample s
 * holds, and hit_i[s] = (c_i[s] >= mk_i), the hit bigsi_hip_search_batch reports at threshold t.  A record with u_i > 0 and a locus l
 * does
 *     records[l]  += 1                                  (uint32)
 *     best[l][s]   = max(best[l][s], key_i[s])          for every selected s with hit_i[s]
 *     hits[l][s]  += 1                                  (uint32) for every such s
 * and a record with u_i == 0 or BIGSI_TYPING_NONE changes nothing.  The key is 64 bits of integer arithmetic only:
 *     score_i[s] = floor(c_i[s] * (2^32 - 1) / u_i)     (uint64: c <= u < 2^32, so the product fits; an exact run has c = u and
 *                                                        score = 2^32 - 1)
 *     key_i[s]   = score_i[s] << 32 | (0xFFFFFFFF - allele_of[i])
 * The best record of a locus in a sample is the one with the highest fraction of its k-mers found; ties go to the lowest allele
 * identity.  The key of a hit is never 0 (its low half is >= 1): best == 0 means "no record of this locus hit this sample".  The
 * allele is 0xFFFFFFFF - (key & 0xFFFFFFFF) and the fraction score / (2^32 - 1).  Two different fractions c_i / u_i and c_j / u_j
 * share a score only when u_i * u_j > 2^32, which allele-sized records never reach; the definition above stands regardless, and
 * every implementation (device, twin, reference) computes exactly it.  Out come
 *     best              n_loci rows of num_cols uint64, hits n_loci rows of num_cols uint32 (either may be NULL: not copied);
 *                       an unselected column holds zeros
 *     locus_counts[l]   { called, exact, multiple }, 3 x uint32 over the selected columns: cells with best != 0, with
 *                       score == 2^32 - 1, and with hits > 1
 *     sample_counts[s]  { called, exact }, 2 x uint32 for s < num_cols, counted over the loci.  An unselected column gets zeros
 *     records[l]        the records of locus l with k-mers
 * Everything is integer max / add / compare: best, hits and every count are bit-identical under any order of the records, any cut
 * into batches or chunks, and from run to run.  A record added twice counts twice in hits and records and changes nothing in best.
 *
 * Limits.  n_loci is at most BIGSI_TYPING_MAX_LOCI, and the cells -- n_loci x ceil(num_cols / 64) x 64 x 12 bytes of device memory,
 * held for the accumulator's life -- at most BIGSI_TYPING_CELL_BYTES.  4 GiB is a DESIGN limit, not a
 * measured one: it is 357 loci at a million samples, and a caller with a larger scheme slices it by locus (every slice an accumulator
 * of its own, a record going to its locus's slice only), as bigsi_amd's BIGSI.typing_arrays does.
 *
 *   typing_create     device cells and counts, zeroed, for the index's num_cols at this moment and the selection.  The accumulator
 *                     belongs to the index: destroy it before bigsi_hip_close.  An index whose num_cols, num_rows or num_hashes
 *                     have changed since gets BIGSI_ERR_STATE from every call but destroy.
 *   typing_reset      zeroes best, hits and records (and makes an accumulator usable again after a failed typing_add_stream).
 *   typing_add_batch  adds a batch of this index whose last run was made with BIGSI_RUN_SKIP_COMPACT (exact or counting, dense or
 *                     BIGSI_RUN_SPARSE_COUNTS: a counter is read only under a hit bit).  locus_of and allele_of (n_entries == the
 *                     batch's n_seqs each) are validated on the host first -- a bad value is BIGSI_ERR_INVALID naming the record,
 *                     and nothing is added -- then uploaded, and k_locus_best is queued on the stream the run finished on.  The
 *                     batch's completion event is recorded again behind it, so bigsi_hip_batch_reload, bigsi_hip_batch_run and
 *                     bigsi_hip_batch_destroy directly afterwards are safe without any synchronisation by the caller, and neither
 *                     label array is read any more when the call returns.  BIGSI_ERR_STATE for a batch of another index and for
 *                     what bigsi_hip_tally_add_batch refuses a batch for.
 *   typing_add_stream any number of host sequences (the arguments of bigsi_hip_search_stream) and their locus_of[n_seqs] and
 *                     allele_of[n_seqs]: cut into device batches by the tally's rule (include/bigsi_hip_tally.h) that alternate
 *                     over two workspaces of the index of the call's own.  A chunk without a k-mer position adds nothing.  On a
 *                     failure the workspaces are destroyed and the accumulator is marked unusable (every call but reset and
 *                     destroy: BIGSI_ERR_STATE).
 *   typing_fetch      waits for everything added so far, counts the cells (every time: a second fetch returns the same; the cells
 *                     keep accumulating afterwards) and copies out.  best / hits may be NULL: that array is not copied.
 *                     BIGSI_ERR_CAPACITY when cell_capacity < n_loci x num_cols (with best or hits asked for) or sample_capacity
 *                     < num_cols: nothing is written.
 * BIGSI_ERR_INVALID: a NULL argument, n_loci == 0 or above BIGSI_TYPING_MAX_LOCI, n_entries != n_seqs, a locus_of value that is
 * neither below n_loci nor BIGSI_TYPING_NONE, an allele_of value above BIGSI_TYPING_MAX_ALLELE, and what a stream's arguments are
 * refused for.  BIGSI_ERR_NOMEM: cells above BIGSI_TYPING_CELL_BYTES.  BIGSI_ERR_STATE: an index without columns.  All calls only
 * read the index: ipc and view handles are fine.  There are no group twins. */
#define BIGSI_TYPING_NONE 0xFFFFFFFFu
#define BIGSI_TYPING_MAX_ALLELE 0xFFFFFFFEu
#define BIGSI_TYPING_MAX_LOCI (1u << 20)
#define BIGSI_TYPING_CELL_BYTES (4ull << 30)

typedef struct bigsi_hip_typing bigsi_hip_typing;
int bigsi_hip_typing_create(bigsi_hip_index *ix, uint32_t n_loci, const uint8_t *columns /* or NULL */, bigsi_hip_typing **out);
int bigsi_hip_typing_destroy(bigsi_hip_typing *t);
int bigsi_hip_typing_reset(bigsi_hip_typing *t);
int bigsi_hip_typing_add_batch(bigsi_hip_typing *t, bigsi_hip_batch *b, const uint32_t *locus_of, const uint32_t *allele_of, uint64_t n_entries);
int bigsi_hip_typing_add_stream(bigsi_hip_typing *t, const char *seqs, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, double threshold,
                                const uint32_t *locus_of, const uint32_t *allele_of);
int bigsi_hip_typing_fetch(bigsi_hip_typing *t, uint64_t *best /* or NULL */, uint32_t *hits /* or NULL */, uint64_t cell_capacity, uint32_t *locus_counts,
                           uint32_t *sample_counts, uint64_t sample_capacity, uint32_t *records);

#ifdef __cplusplus
}
#endif

#endif /* BIGSI_HIP_TYPING_H */
