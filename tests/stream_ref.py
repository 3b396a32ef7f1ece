"""The cut rule of the streamed search (bigsi_hip_search_stream, _ranked, _scored) restated in plain Python, written from the loop
of search_stream_impl as it stood before the rule moved into bigsi_amd/csrc/bigsi_launch.hpp -- and, for the band decision the loop
asks for, the `taken` and launch count of plan_band_sweep.  tests/test_stream_plan_host.py compares it with the compiled header;
the GPU tests (tests/test_gpu_stream_cuts.py, tests/test_gpu_parity.py) compare it with what bigsi_hip_stream_last_chunks reports.
No numpy tricks, no sharing of code with the library: loops over integers."""

CHUNK_POSITIONS = 1 << 20            # exact and scored streams
LARGE_CHUNK_POSITIONS = 1 << 22      # thresholded streams, and the exact chunk tried for the band sweep
CHUNK_SEQS = 4096
SLOTS = 4                            # workspaces in flight


def ceil_div(a, b):
    return -(-a // b)


def limits(threshold, scored=False, force_counts=False, chunk_positions=0, large_chunk_positions=0, chunk_seqs=0):
    """dict(small_pos, large_pos, seqs, small_chunks, band_chunks, chunk_pos); an override of 0 keeps the library's value, and the
    sequence cap is never raised above the library's"""
    small = chunk_positions or CHUNK_POSITIONS
    large = large_chunk_positions or LARGE_CHUNK_POSITIONS
    seqs = min(chunk_seqs, CHUNK_SEQS) if chunk_seqs else CHUNK_SEQS
    small_chunks = threshold == 1.0 or bool(scored)
    band_chunks = threshold == 1.0 and not scored and not force_counts
    return dict(small_pos=small, large_pos=large, seqs=seqs, small_chunks=small_chunks, band_chunks=band_chunks,
                chunk_pos=small if small_chunks else large)


class DecreasingOffsets(ValueError):
    pass


def chunk_end(offsets, n_seqs, nxt, k, limit_pos, limit_seqs):
    """(end, pos, max_pos) of the chunk that starts at sequence nxt; DecreasingOffsets where the library answers BIGSI_ERR_INVALID"""
    pos, end, max_pos = 0, nxt, 0
    while end < n_seqs and end - nxt < limit_seqs:
        if offsets[end + 1] < offsets[end]:
            raise DecreasingOffsets(end)
        length = offsets[end + 1] - offsets[end]
        n = length - k + 1 if length >= k else 0
        if end > nxt and pos + n > limit_pos:
            break
        pos += max(n, 1)
        max_pos = max(max_pos, n)
        end += 1
    return end, pos, max_pos


def exact_launch_queries(wv):
    """queries per row-AND launch of a large exact batch on results of wv words (exact_launch for 256-thread workgroups)"""
    if wv == 0:
        return 8
    blocks_per_q = ceil_div(wv, 512)
    waves_per_q = ceil_div(wv, 128)
    kb = ceil_div(ceil_div(1600 * blocks_per_q, waves_per_q), 256) * 256
    return max(8, (kb // blocks_per_q) // 8 * 8)


def round_to_launches(n, launch_q, more_follow, exact, band):
    if exact and not band and more_follow and n >= 2 * launch_q:
        return n // launch_q * launch_q
    return n


def band_plan(n_seqs, wv, max_pos, h, m, forced=False, windows=0, segs=0, exact=True, no_sort=False, early_exit=False):
    """(taken, n_launches) of plan_band_sweep"""
    if not exact or early_exit or no_sort or n_seqs == 0 or wv == 0 or m == 0:
        return False, 0
    W = min(windows, 1 << 16) if windows else (1 if n_seqs <= 4096 else 4)
    S = min(segs, 2) if segs else 1
    n_segs = ceil_div(wv, 128)
    waves = n_seqs * S
    groups = ceil_div(n_segs, S)
    grid = ceil_div(waves, 4)
    in_flight = waves * 2 * 1024
    if grid > 0x7FFFFFFF or groups * W > 0x7FFFFFFF:
        return False, 0
    if not forced:
        all_waves = n_seqs * n_segs
        slices = 1 if all_waves >= 1024 else min(64, ceil_div(2048, max(all_waves, 1)), max(max_pos // 16, 1))
        want_sorted = all_waves >= 1024 and max_pos * h >= 1024
        if slices != 1 or not want_sorted or n_seqs * max_pos * h < m or n_seqs < 3072 or in_flight > 16 << 20:
            return False, 0
    if not segs and W == 1 and n_segs >= 2 and wv - (n_segs - 1) * 128 <= 32 and 2 * in_flight <= 16 << 20:
        groups -= 1
    return True, groups * W


def cuts(lengths, k, threshold, n_cols, h, m, scored=False, flags_force_counts=False, flags_band_sweep=False, flags_no_sort=False,
         flags_early_exit=False, chunk_positions=0, large_chunk_positions=0, chunk_seqs=0, band_windows=0, band_segs=0):
    """The chunks of one stream call over sequences of these lengths on an index of n_cols columns, h hashes and m rows: a list of
    (first sequence, band, n sequences, max_pos).  The loop also drops the band chunk when the device is short of free memory for its row lists:
    not restated (the inputs of the tests need a few hundred megabytes at most)."""
    offsets = [0]
    for n in lengths:
        offsets.append(offsets[-1] + n)
    return cuts_of_offsets(offsets, k, threshold, n_cols, h, m, scored, flags_force_counts, flags_band_sweep, flags_no_sort, flags_early_exit,
                           chunk_positions, large_chunk_positions, chunk_seqs, band_windows, band_segs)


def cuts_of_offsets(offsets, k, threshold, n_cols, h, m, scored=False, flags_force_counts=False, flags_band_sweep=False, flags_no_sort=False,
                    flags_early_exit=False, chunk_positions=0, large_chunk_positions=0, chunk_seqs=0, band_windows=0, band_segs=0):
    n_seqs = len(offsets) - 1
    lim = limits(threshold, scored, flags_force_counts, chunk_positions, large_chunk_positions, chunk_seqs)
    wv = ceil_div(n_cols, 64)
    launch_q = exact_launch_queries(wv)
    out, nxt = [], 0
    while nxt < n_seqs:
        band = False
        if lim["band_chunks"]:
            end, pos, max_pos = chunk_end(offsets, n_seqs, nxt, k, lim["large_pos"], lim["seqs"])
            band = not flags_force_counts and band_plan(end - nxt, wv, max_pos, h, m, flags_band_sweep, band_windows, band_segs,
                                                        no_sort=flags_no_sort, early_exit=flags_early_exit)[0]
        if not band:
            end, pos, max_pos = chunk_end(offsets, n_seqs, nxt, k, lim["chunk_pos"], lim["seqs"])
        end = nxt + round_to_launches(end - nxt, launch_q, end < n_seqs, threshold == 1.0, band)
        out.append((nxt, band, end - nxt, max_pos))
        nxt = end
    return out
