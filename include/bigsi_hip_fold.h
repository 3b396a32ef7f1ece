/*
 * bigsi_hip_fold.h -- row folding of libbigsi_hip.so: the same index under a SMALLER Bloom filter, without the source data.
 *
 * Part of the MAINTENANCE layer of the C ABI (include/bigsi_hip.h, include/bigsi_hip_compact.h): single-index entry points in those
 * headers' conventions (return codes, bigsi_hip_last_error, one thread per handle, the row format).  A header of its own because
 * bigsi_hip.h is kept to 60 entry points and bigsi_hip_compact.h to its three (tests/test_abi_and_host.py and
 * tests/test_compact_columns_host.py pin both): the Python binding lists these in FOLD_SIGNATURES.
 */
#ifndef BIGSI_HIP_FOLD_H
#define BIGSI_HIP_FOLD_H

#include "bigsi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Row folding.  A k-mer's row is floor_mod(signed murmur3(kmer, seed), num_rows) (the reference's bloom/bloomfilter.py:5-6), and for
 * a divisor m' of m, floor_mod(x, m) mod m' == floor_mod(x, m').  So with m' = m / factor
 *     row'[r] = row[r] | row[r + m'] | row[r + 2 m'] | ... | row[r + (factor - 1) m']        for r in [0, m')
 * is bit for bit the matrix the same samples build under num_rows = m': rows, search results, counts and scores all match, no false
 * negative appears, and the false-positive rate rises (bigsi_hip_column_popcounts of the folded index says by how much).  Bits at
 * columns >= num_cols (bigsi_hip_set_rows can put them there) are zero in every folded row.  A NULL index: BIGSI_ERR_INVALID.
 *   fold_rows       in place: num_rows becomes num_rows / factor; *new_num_rows = that (may be NULL).  factor == 1 is a no-op that
 *                   touches nothing.  factor == 0, or a factor that does not divide num_rows: BIGSI_ERR_INVALID.  A writer: ipc / view
 *                   handles get BIGSI_ERR_STATE, and so does an owner while views of it are open (their row count would go stale).
 *                   The allocation keeps its size (bigsi_hip_trim_rows gives the memory back); bigsi_hip_get_info and the exports
 *                   report the new num_rows, never the allocation's.
 *   fold_rows_into  out of place: dst becomes src folded by src's num_rows / dst's num_rows, which must be an integer >= 1 (1: a
 *                   plain copy of the rows).  dst != src, same device, same num_hashes (BIGSI_ERR_INVALID otherwise); dst must be
 *                   writable and hold no columns (BIGSI_ERR_STATE otherwise); its capacity grows to src's num_cols
 *                   (bigsi_hip_reserve_cols) and it ends with src's num_cols.  src is only read and may be a view or an ipc handle.
 *                   While views of dst are open the call is refused as well (BIGSI_ERR_STATE: their column count would go
 *                   stale).  Both handles are held for the duration of the call (one thread per handle): BIGSI_ERR_STATE when
 *                   another host thread is inside src.
 *   trim_rows       the row counterpart of bigsi_hip_shrink_to_fit: when the allocation holds more rows than num_rows (after a
 *                   fold_rows), move the matrix into an allocation of num_rows x stride and free the old one.  ipc / view handles
 *                   get BIGSI_ERR_STATE (they do not know the owner's allocation); for the owner a no-op when nothing is to be
 *                   gained, otherwise a writer that moves the matrix: BIGSI_ERR_STATE while views are open.  Needs room for the
 *                   smaller copy beside the matrix while it runs: BIGSI_ERR_NOMEM leaves the index as it was.
 * Batches of the index stay valid, as across bigsi_hip_set_num_cols and the compaction calls: every run takes the index's geometry
 * at that moment, so a batch created before a fold and run after it gives the folded index's answers; results of a run made BEFORE
 * the call must be fetched (or dropped) first.  There are no group twins: folding the column shards of a device group is the same
 * sweep per shard, a straightforward follow-up that has had no multi-GPU hardware to run on. */
int bigsi_hip_fold_rows(bigsi_hip_index *ix, uint64_t factor, uint64_t *new_num_rows);
int bigsi_hip_fold_rows_into(bigsi_hip_index *dst, const bigsi_hip_index *src);
int bigsi_hip_trim_rows(bigsi_hip_index *ix);

#ifdef __cplusplus
}
#endif

#endif /* BIGSI_HIP_FOLD_H */
