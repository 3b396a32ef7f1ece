/*
 * bigsi_hip_kmercount.h -- the exact k-mer counter of libbigsi_hip.so: reads go in, in any number of calls; out come the abundance
 * spectrum and the Bloom filter of the k-mers seen at least C times, so that a sample's filter is made from raw sequencing data with
 * the k-mers of sequencing errors left out.  The counting, the spectrum and the filter run on the device (k_count_kmers and
 * k_kmer_table_*: an open-addressing table in HBM).
 *
 * The semantics are the SEMANTICS block of include/bigsi_cpu_kmercount.h, unchanged, and the entry points have that header's
 * signatures and return codes (bigsi_hip_last_error holds the message): k in [1, 32], acgt folded, a window with any other byte
 * skipped, canonical keys packed 2 bits per base, exact uint32 counts under a lifetime bound of 2^32 - 1 positions, the 256-bin
 * spectrum, and the filter byte for byte bigsi_hip_bloom of the kept k-mers.  Results are a function of the multiset of sequences only.
 * What differs from the host twin:
 *   create   `device` is the GPU the counter lives on; `expected_distinct` sizes the first table (twice the hint, a power of two;
 *            0: the library's own start).  The table grows by itself: before a chunk of a call is counted it holds at most half as
 *            many keys as slots, whatever the chunk brings.
 *   add      validates and cuts the call from the offsets alone, before any byte behind `seqs` is read (BIGSI_ERR_INVALID for
 *            offsets that decrease, BIGSI_ERR_RANGE for the call that would pass the lifetime bound: nothing of it is counted).  An
 *            accepted call reads exactly seqs[offsets[0] .. offsets[n_seqs]).  Returns when the input is no longer read and counted.
 *   info     out[3] is the table's slot count.
 *   fetch    ascending key order.
 *   failure  an allocation failure while the table grows returns BIGSI_ERR_NOMEM, any other device failure inside add its own code;
 *            either leaves the counter refusing everything but reset and destroy with BIGSI_ERR_STATE.  So does a reset that cannot
 *            allocate its table (BIGSI_ERR_NOMEM): a later reset tries again.  A host allocation failure inside add (before anything
 *            is counted) or fetch returns BIGSI_ERR_NOMEM and leaves the counter as it was.
 * One host thread per counter at a time.  Header of its own for the reason bigsi_hip_tally.h gives; the Python binding lists these in
 * KMERCOUNT_SIGNATURES.
 */
#ifndef BIGSI_HIP_KMERCOUNT_H
#define BIGSI_HIP_KMERCOUNT_H

#include "bigsi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef BIGSI_KMERCOUNT_MAX_K
#define BIGSI_KMERCOUNT_MAX_K 32u
#endif

typedef struct bigsi_hip_kmer_counter bigsi_hip_kmer_counter;

int bigsi_hip_kmer_counter_create(int device, uint32_t k, uint64_t expected_distinct, bigsi_hip_kmer_counter **out);
int bigsi_hip_kmer_counter_destroy(bigsi_hip_kmer_counter *c);
int bigsi_hip_kmer_counter_reset(bigsi_hip_kmer_counter *c);
/* Count the k-mers of n_seqs sequences (seqs + offsets[i] .. offsets[i + 1]; n_seqs = 0 is allowed and counts nothing). */
int bigsi_hip_kmer_counter_add(bigsi_hip_kmer_counter *c, const char *seqs, const uint64_t *offsets, uint64_t n_seqs);
/* out[0] positions counted, out[1] positions skipped (windows with a byte other than ACGTacgt), out[2] distinct keys, out[3] table slots. */
int bigsi_hip_kmer_counter_info(bigsi_hip_kmer_counter *c, uint64_t out[4]);
int bigsi_hip_kmer_counter_spectrum(bigsi_hip_kmer_counter *c, uint64_t out[256]);
/* The entries in ascending key order: *n of them.  capacity < *n is a sizing call: BIGSI_ERR_CAPACITY, *n set, nothing written
 * (keys and counts may then be NULL). */
int bigsi_hip_kmer_counter_fetch(bigsi_hip_kmer_counter *c, uint64_t *keys, uint32_t *counts, uint64_t capacity, uint64_t *n);
/* out: ceil(m / 8) bytes in the row byte format of bigsi_hip_bloom, zeroed by the call.  min_count == 0, m == 0, h == 0: BIGSI_ERR_INVALID. */
int bigsi_hip_kmer_counter_bloom(bigsi_hip_kmer_counter *c, uint64_t m, uint32_t h, uint32_t min_count, uint8_t *out);

#ifdef __cplusplus
}
#endif

#endif /* BIGSI_HIP_KMERCOUNT_H */
