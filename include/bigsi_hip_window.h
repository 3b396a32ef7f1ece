/*
 * bigsi_hip_window.h -- windowed search of libbigsi_hip.so: per sample the best window of W k-mer positions of a query, and where on
 * the query the windows that pass lie.
 *
 * Part of the QUERY layer of the C ABI (include/bigsi_hip.h): entry points in that header's conventions (return codes,
 * bigsi_hip_last_error, one thread per handle, the row format).  A header of its own because bigsi_hip.h is kept to 60 entry points
 * (tests/test_abi_and_host.py pins it): the Python binding lists these in WINDOW_SIGNATURES.
 */
#ifndef BIGSI_HIP_WINDOW_H
#define BIGSI_HIP_WINDOW_H

#include "bigsi_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BIGSI_WINDOW_MAX 65535u      /* the largest window, in k-mer positions (16 counting planes) */

/* One record per hit, beside its colour. */
typedef struct {
    uint32_t best_found;      /* max_s found(c, s)                                  */
    uint32_t best_start;      /* the LOWEST s that reaches it                       */
    uint32_t first_start;     /* lowest  s with found(c, s) >= need                 */
    uint32_t last_start;      /* highest s with found(c, s) >= need                 */
    uint32_t windows_passing; /* number of s with found(c, s) >= need               */
    uint32_t reserved;        /* 0                                                  */
} bigsi_hip_window_hit;

/* Windowed search: a local question where a search asks a global one.  Sequence i of a batch has n = max(len - k + 1, 0) k-mer
 * positions; for position p let A_p be the AND of the h rows of the k-mer at p (canonicalised and hashed as a search does),
 * restricted to the columns < num_cols (bits that bigsi_hip_set_rows put behind num_cols never count).  Counting is BY POSITION: a
 * k-mer that occurs twice in a window counts twice, as in the presence strings (not by unique k-mer, as a search counts).  With
 * `window` = W >= 1 positions and 0 < threshold <= 1, per sequence
 *     We   = min(W, n)                      -> window_used[i]
 *     need = ceil(We * threshold)           -> need[i]           (one IEEE double multiply, as Python's math.ceil(We * t))
 *     found(c, s) = number of p in [s, s + We) where A_p has bit c,   for every window start s in [0, n - We]
 * and column c is a hit of sequence i when max_s found(c, s) >= need.  A sequence with n = 0 has no window and no hit
 * (window_used = need = 0).  Hits per sequence are in ascending colour, hit_offsets as bigsi_hip_batch_fetch_hits writes them; each
 * hit carries one bigsi_hip_window_hit.  Positions [first_start, last_start + We) are the extent of the match on the query.
 *   window_search        one call, host sequences in, host hit lists out (the arguments of bigsi_hip_search_batch).  The sequences
 *                        are staged into a workspace of the index that lives until bigsi_hip_close and run as an exact search
 *                        first, as bigsi_hip_kmer_prevalence does and for the same reason (the exact row-AND is the cheapest run
 *                        that leaves K1's row ids behind on every route), so an index without columns gets BIGSI_ERR_STATE as a
 *                        search does.  COST of that pass: one read of every unique k-mer's h rows on top of the sweep -- the
 *                        sweep itself reads 2 h rows per window start plus We h rows per segment of starts, so the exact pass is
 *                        about a third on top of a long query and more than that on a batch of queries shorter than the window.
 *   batch_window_search  the same for a batch that has completed a run of any kind (BIGSI_ERR_STATE otherwise, as
 *                        bigsi_hip_batch_kmer_prevalence).  BIGSI_ERR_STATE too for a batch of explicit k-mers
 *                        (bigsi_hip_batch_create_elements) and when num_hashes changed since the run.  The batch's own results
 *                        (hit lists, counters, bit vectors) are left as they are.
 * BIGSI_ERR_CAPACITY when capacity < hit_offsets[n_seqs], bigsi_hip_batch_fetch_hits' protocol: hit_offsets, window_used and need
 * are filled, colours and records are untouched.
 * BIGSI_ERR_INVALID: window == 0 or window > BIGSI_WINDOW_MAX, a threshold that is not in (0, 1], a NULL window_used, need or
 * hit_offsets, NULL colours or records with capacity > 0, what a batch's arguments are refused for (NULL pointers, n_seqs == 0,
 * k == 0, descending offsets), and a sweep too large for one launch (more than 2^31 - 1 workgroups, or per-segment maxima above
 * 2 GiB: the message carries the numbers).
 * Every record is computed twice on the device, by two kernels that share no arithmetic (the bit-sliced sliding maximum, and a
 * popcount walk over the hit's presence bits); the library compares the two best_found values after copy-out and returns
 * BIGSI_ERR_STATE with a message naming the hit should they ever differ: it never hands out a record it could not confirm.
 * Both calls only read the index: ipc and view handles are fine.  There are no group twins. */
int bigsi_hip_window_search(bigsi_hip_index *ix, const char *seqs, const uint64_t *offsets, uint32_t n_seqs, uint32_t k,
                            uint32_t window, double threshold, uint32_t *window_used /* n_seqs */, uint32_t *need /* n_seqs */,
                            uint64_t *hit_offsets /* n_seqs + 1 */, uint32_t *colours, bigsi_hip_window_hit *records,
                            uint64_t capacity /* entries of colours / records */);
int bigsi_hip_batch_window_search(bigsi_hip_batch *b, uint32_t window, double threshold, uint32_t *window_used, uint32_t *need,
                                  uint64_t *hit_offsets, uint32_t *colours, bigsi_hip_window_hit *records, uint64_t capacity);

#ifdef __cplusplus
}
#endif

#endif /* BIGSI_HIP_WINDOW_H */
