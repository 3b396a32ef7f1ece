/*
 * bigsi_cpu_kmercount.h -- libbigsi_cpu.so: an exact k-mer counter on the host.  Reads go in, in any number of calls; out come the
 * abundance spectrum and the Bloom filter of the k-mers seen at least C times -- byte for byte the filter bigsi_cpu_bloom (and
 * bigsi_hip_bloom) makes from the same k-mer list, so that a sample's filter can be made from raw sequencing data with the k-mers of
 * sequencing errors (seen once) left out.  Implemented plainly (a map, bigsi_cpu_bloom's hashing) for hosts without a GPU and as
 * the definition the device counter of libbigsi_hip.so (include/bigsi_hip_kmercount.h: the same entry points, counted in a hash table
 * in HBM) is held against.  Entry points in the conventions of bigsi_cpu.h (return codes, bigsi_cpu_last_error).
 *
 * SEMANTICS (tests/kmercount_ref.py restates them):
 *   k        1 <= k <= 32 (BIGSI_ERR_INVALID beyond: a key is one 64-bit word).
 *   case     a c g t count as A C G T.
 *   windows  a window of k bytes that holds any other byte is skipped, not counted; a sequence shorter than k contributes nothing.
 *   key      the canonical k-mer -- the lexicographic minimum of the window and its reverse complement -- packed 2 bits per base
 *            (A 0, C 1, G 2, T 3), the first base in the highest used bits: the numeric minimum is the lexicographic one.  A
 *            palindromic window counts once per occurrence; a k-mer seen forward in one read and reverse-complemented in another is
 *            one key.  ~0 is no canonical key for k <= 32 (T^32 is A^32 = 0); key 0 is a real k-mer.
 *   counts   per key an exact uint32 number of occurrences.  A counter takes at most 2^32 - 1 positions (windows, skipped ones
 *            included) in its lifetime (BIGSI_ERR_RANGE for the call that would pass it: nothing of that call is counted, and no
 *            byte of it is read), so no count wraps.
 *   spectrum spectrum[c], c in 1..255: distinct keys with count c; bin 255 also holds every count above; bin 0 is 0.
 *   filter   for (m, h, min_count >= 1): the OR, over the keys with count >= min_count, of the h bits bigsi_cpu_bloom sets for the
 *            k-mer's upper-case ASCII string (same MurmurHash3, same floor-mod row, same byte and bit order).
 * Results are a function of the multiset of sequences only: the same however the input is cut into calls, in any order.
 */
#ifndef BIGSI_CPU_KMERCOUNT_H
#define BIGSI_CPU_KMERCOUNT_H

#include "bigsi_cpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BIGSI_KMERCOUNT_MAX_K 32u

typedef struct bigsi_cpu_kmer_counter bigsi_cpu_kmer_counter;

/* `device` and `expected_distinct` (a sizing hint) are the device counter's, which has the same shape; the host ignores both. */
int bigsi_cpu_kmer_counter_create(int device, uint32_t k, uint64_t expected_distinct, bigsi_cpu_kmer_counter **out);
int bigsi_cpu_kmer_counter_destroy(bigsi_cpu_kmer_counter *c);
int bigsi_cpu_kmer_counter_reset(bigsi_cpu_kmer_counter *c);
/* Count the k-mers of n_seqs sequences (seqs + offsets[i] .. offsets[i + 1]; n_seqs = 0 is allowed and counts nothing). */
int bigsi_cpu_kmer_counter_add(bigsi_cpu_kmer_counter *c, const char *seqs, const uint64_t *offsets, uint64_t n_seqs);
/* out[0] positions counted, out[1] positions skipped (windows with a byte other than ACGTacgt), out[2] distinct keys, out[3] 0
 * (a device counter's table slots). */
int bigsi_cpu_kmer_counter_info(bigsi_cpu_kmer_counter *c, uint64_t out[4]);
int bigsi_cpu_kmer_counter_spectrum(bigsi_cpu_kmer_counter *c, uint64_t out[256]);
/* The entries in ascending key order: *n of them.  capacity < *n is a sizing call: BIGSI_ERR_CAPACITY, *n set, nothing written
 * (keys and counts may then be NULL). */
int bigsi_cpu_kmer_counter_fetch(bigsi_cpu_kmer_counter *c, uint64_t *keys, uint32_t *counts, uint64_t capacity, uint64_t *n);
/* out: ceil(m / 8) bytes in the row byte format of bigsi_cpu_bloom, zeroed by the call.  min_count == 0, m == 0, h == 0: BIGSI_ERR_INVALID. */
int bigsi_cpu_kmer_counter_bloom(bigsi_cpu_kmer_counter *c, uint64_t m, uint32_t h, uint32_t min_count, uint8_t *out);

#ifdef __cplusplus
}
#endif

#endif /* BIGSI_CPU_KMERCOUNT_H */
