"""Per-workload kernel measurements behind DESIGN.md section 5 / profiles/*.json (one JSON object per line on stdout).

    python scripts/measure.py [c2stream] [c3batch] [p16] [c4shard] [northstar] [k5] [transpose] [colpop] [compact] [fold] [prevalence] [collapse] [consensus] [pairwise] [tally] [classify] [associate] [genotype] [typing] [window] ...

Every figure is a HIP-event duration recorded by the library around its own kernels (bigsi_hip_set_profiling) over
`reps` launches; run the same command under `rocprofv3 --kernel-trace --stats` for the per-kernel table that goes to
profiles/.  Algorithmic bytes follow SURVEY.md section 8d: unique rows x ceil(N/64) x 8 + result vectors."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bigsi_amd import _lib  # noqa: E402
from bigsi_amd._lib import check  # noqa: E402
from bigsi_amd.storage import get_storage  # noqa: E402

SEED = 20260928
PEAK = 8000.0


def open_index(name, m, n_cols, h, draws=2, k=31):
    st = get_storage({"storage-engine": "hip-hbm", "k": k, "m": m, "h": h,
                      "storage-config": {"name": name, "device": 0, "max_cols": n_cols}})
    st.delete_all()
    for key, v in (("number_of_rows", m), ("number_of_cols", n_cols), ("ksi:bloomfilter_size", m), ("ksi:num_hashes", h)):
        st.set_integer(key, v)
    t0 = time.time()
    st.fill_synthetic(SEED, 0, draws)
    return st, time.time() - t0


def rand_seqs(rng, n, qlen):
    a = rng.integers(0, 4, size=(n, qlen), dtype=np.uint8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [lut[r].tobytes().decode("ascii") for r in a]


def stats(st, reset=1):
    s = _lib.Stats()
    check(_lib.lib().bigsi_hip_stats(st.handle, _lib.C.byref(s), reset))
    return s


def alg_bytes(batch, n_seqs, n_cols):
    _, nu, _ = batch.unique()
    wv = -(-n_cols // 64)
    rows = 0
    for i in range(n_seqs):
        rows += np.unique(batch.rows(i, nu[i])).size
    return int(nu.sum()), rows, rows * wv * 8 + n_seqs * wv * 8


def run_steps(st, batches, threshold, reps, warm=3, prof=2, **kw):
    """(wall ms/step, Stats) over `reps` steps cycling through `batches`."""
    L = _lib.lib()
    for i in range(warm):
        batches[i % len(batches)].run(threshold, **kw)
    check(L.bigsi_hip_synchronize(st.handle))
    check(L.bigsi_hip_set_profiling(st.handle, prof))
    stats(st)
    t0 = time.perf_counter()
    for i in range(reps):
        batches[i % len(batches)].run(threshold, **kw)
    check(L.bigsi_hip_synchronize(st.handle))
    wall = (time.perf_counter() - t0) / reps * 1e3
    s = stats(st)
    check(L.bigsi_hip_set_profiling(st.handle, 0))
    return wall, s


def stride_for(cols):
    """The row stride in bytes the library gives an index of `cols` columns (whole 128-byte lines)."""
    return max(16, -(-(-(-cols // 64)) // 16) * 16) * 8


def timed(fn):
    """Wall-clock ms of one C call that must succeed."""
    t0 = time.perf_counter()
    check(fn())
    return (time.perf_counter() - t0) * 1e3


def get_rows(handle, ids, rb):
    out = np.zeros((ids.size, rb), np.uint8)
    check(_lib.lib().bigsi_hip_get_rows(handle, _lib.ptr(ids), ids.size, _lib.ptr(out), rb))
    return out


def emit(name, **kw):
    kw = dict(workload=name, **kw)
    print(json.dumps(kw), flush=True)


def kernel_line(name, st, batches, n_cols, threshold, reps, note="", **kw):
    nseq = batches[0].n
    wall, s = run_steps(st, batches, threshold, reps, prof=2, **kw)            # row-AND kernel only: clean step time
    _, s1 = run_steps(st, batches, threshold, min(reps, 20), prof=1, **kw)     # every kernel group (event overhead in the step)
    lookups, rows, ab = alg_bytes(batches[0], nseq, n_cols)
    k2 = s.and_ms / reps                                    # row-AND time per step (large batches: several launches)
    r1 = min(reps, 20)
    emit(name, threshold=threshold, n_seqs=nseq, distinct_batches=len(batches), step_ms=wall, k2_ms=k2,
         k2_launches_per_step=s.and_launches / reps, k1_ms=s1.kmerize_ms / r1, k4_ms=s1.compact_ms / r1,
         lookups_per_batch=lookups, unique_rows=rows, alg_bytes=ab, GBps=ab / k2 / 1e6, frac=ab / k2 / 1e6 / PEAK,
         lookups_per_s=lookups / wall * 1e3, note=note)


def c2stream():
    """BASELINE configs[1] with a DIFFERENT batch every step: 32 staged batches of 1000 random 61-mers cycle, so the rows of
    a step (117 MB) are not the rows the previous steps left in the 256 MiB Infinity Cache."""
    m, n, h = 1_000_000, 10_000, 3
    st, _ = open_index("c2", m, n, h)
    rng = np.random.default_rng(7)
    same = [st.new_batch(rand_seqs(np.random.default_rng(1), 1000, 61), 31)]
    many = [st.new_batch(rand_seqs(rng, 1000, 61), 31) for _ in range(32)]
    for thr in (1.0, 0.4):
        kernel_line("c2_same_batch", st, same, n, thr, 200, note="one batch repeated: rows are cache resident")
        kernel_line("c2_stream", st, many, n, thr, 320, note="32 distinct batches cycling")
    for b in same + many:
        b.close()
    st.delete_all()


def c3batch():
    """C3 index; 256 vs 2048 vs 8192 queries per launch (does the address-ordered sweep survive a grid that is not co-resident?)."""
    m, n, h = 10_000_000, 100_000, 4
    st, _ = open_index("c3", m, n, h)
    rng = np.random.default_rng(1)
    for nq in (256, 2048, 8192):
        bs = [st.new_batch(rand_seqs(rng, nq, 1000), 31) for _ in range(2)]
        for thr in (1.0, 0.4):
            kernel_line("c3_batch%d" % nq, st, bs, n, thr, max(4, 5120 // nq), sparse_counts=True)
        for b in bs:
            b.close()
    st.delete_all()


def p16():
    """Counting kernel with P=16 planes (1024..65535 k-mers per query): 256 x 2 kbp and 128 x 4 kbp at t=0.4 vs exact."""
    m, n, h = 10_000_000, 100_000, 4
    st, _ = open_index("c3", m, n, h)
    rng = np.random.default_rng(3)
    for nq, ql in ((256, 1000), (256, 2000), (128, 4000), (64, 8000)):
        bs = [st.new_batch(rand_seqs(rng, nq, ql), 31) for _ in range(2)]
        for thr in (1.0, 0.4):
            kernel_line("c3_q%dbp" % ql, st, bs, n, thr, 12, sparse_counts=True)
        for b in bs:
            b.close()
    st.delete_all()


def shard(name, m, n, h):
    st, fill = open_index(name, m, n, h)
    rng = np.random.default_rng(1)
    bs = [st.new_batch(rand_seqs(rng, 256, 1000), 31) for _ in range(2)]
    for thr in (1.0, 0.4):
        kernel_line(name, st, bs, n, thr, 20, note="fill %.2f s" % fill, sparse_counts=True)
    for b in bs:
        b.close()
    st.delete_all()


def c4shard():
    shard("c4_shard_25Mx62500_h3", 25_000_000, 62_500, 3)


def northstar():
    shard("northstar_shard_10Mx62500_h3", 10_000_000, 62_500, 3)
    shard("northstar_shard_10Mx62500_h4", 10_000_000, 62_500, 4)


def k5():
    """Presence strings (score=True) at scale: 64 x 1 kbp queries on a 10M x 62.5k shard, each planted (70 % of its k-mers)
    into H samples, H = 16 .. 4096 per query -> up to 262k hits per batch; bigsi_hip_batch_presence_hits, kernel time from
    the library's events, whole-call time (host pair lists + H2D + kernels + D2H of the strings) from the wall clock."""
    m, n, h = 10_000_000, 62_500, 3
    st, _ = open_index("k5", m, n, h)
    rng = np.random.default_rng(11)
    seqs = rand_seqs(rng, 64, 1000)
    L = _lib.lib()
    done = 0
    for H in (16, 256, 4096):
        for qi, s in enumerate(seqs):
            for c in rng.choice(n, size=H - done, replace=False):
                st.insert_kmers(int(c), [s[:700]], 31)
        done = H
        b = st.new_batch(seqs, 31)
        b.run(0.4, sparse_counts=True)
        off, col, cnt = b.hits()
        nk, nu, _ = b.unique()
        b.presence_hits(off, col, nk)                      # warm (allocations)
        check(L.bigsi_hip_set_profiling(st.handle, 1))
        stats(st)
        reps = 3
        t0 = time.perf_counter()
        for _ in range(reps):
            blob, starts, lens = b.presence_hits(off, col, nk)
        dt = (time.perf_counter() - t0) / reps
        s_ = stats(st)
        check(L.bigsi_hip_set_profiling(st.handle, 0))
        kms = s_.presence_ms / max(s_.presence_launches, 1)
        ab = s_.presence_bytes / max(s_.presence_launches, 1)
        for t in range(8):
            assert int((blob[int(starts[t]):int(starts[t] + lens[t])] == ord("1")).sum()) >= 670
        emit("k5_presence_hits", n_seqs=len(seqs), hits=int(off[-1]), positions=int(nk[0]), kernels_ms=kms, call_ms=dt * 1e3,
             alg_bytes=ab, GBps=ab / kms / 1e6, frac=ab / kms / 1e6 / PEAK, string_bytes=int(lens.sum()),
             note="k_presence_bits + k_presence_expand; alg bytes = unique k-mers x h x 8 x distinct hit words + string bytes")
        # K6: the same hits through bigsi_hip_batch_score_hits -- packed presence bits + score records instead of ASCII strings
        b.score_hits(off, col, cnt, nk)
        check(L.bigsi_hip_set_profiling(st.handle, 1))
        stats(st)
        t0 = time.perf_counter()
        for _ in range(reps):
            rec, pbits, boff = b.score_hits(off, col, cnt, nk)
        dt = (time.perf_counter() - t0) / reps
        s_ = stats(st)
        check(L.bigsi_hip_set_profiling(st.handle, 0))
        kms = s_.presence_ms / max(s_.presence_launches, 1)
        ab = s_.presence_bytes / max(s_.presence_launches, 1)
        from bigsi_amd.graph.bigsi import scored_rows
        t0 = time.perf_counter()
        rows = scored_rows(rec, pbits, boff, np.repeat(nk.astype(np.int64), np.diff(off.astype(np.int64))), n)
        host_s = time.perf_counter() - t0
        assert len(rows) == int(off[-1]) and rows[0][2].count("1") >= 670
        emit("k6_score_hits", n_seqs=len(seqs), hits=int(off[-1]), positions=int(nk[0]), kernels_ms=kms, call_ms=dt * 1e3,
             alg_bytes=ab, GBps=ab / kms / 1e6, frac=ab / kms / 1e6 / PEAK, presence_bits_bytes=int(boff[-1]), score_bytes=int(rec.nbytes),
             host_rows_ms=host_s * 1e3, host_us_per_hit=host_s / max(int(off[-1]), 1) * 1e6,
             note="k_presence_bits + k_presence_score; alg bytes = unique k-mers x h x 8 x distinct hit words + packed bits + score records; "
                  "host_rows = closed-form fields + presence strings for all hits (scored_rows)")
        b.close()
    st.delete_all()


def transpose():
    """Bloom filters -> matrix columns (the build transpose): filters resident in device memory
    (bigsi_hip_insert_columns_device), kernel time from the library's events; bytes = filters in + rows out."""
    import torch
    L = _lib.lib()
    shapes = ((10_000_000, 8192), (1_000_000, 100_000), (1_000_000, 100_000 - 37))
    if os.environ.get("BIGSI_TR_SHAPES"):          # e.g. "4000000x16384,2000000x32768"
        shapes = tuple(tuple(int(x) for x in sh.split("x")) for sh in os.environ["BIGSI_TR_SHAPES"].split(","))
    for m, ncols in shapes:
        st = get_storage({"storage-engine": "hip-hbm", "k": 31, "m": m, "h": 3,
                          "storage-config": {"name": "tr", "device": 0, "max_cols": ncols}})
        st.delete_all()
        for key, v in (("number_of_rows", m), ("number_of_cols", 0), ("ksi:bloomfilter_size", m), ("ksi:num_hashes", 3)):
            st.set_integer(key, v)
        nb = (m + 7) // 8
        align = int(os.environ.get("BIGSI_TR_PITCH_ALIGN", "128"))      # the library stages host filters at a 128-byte pitch (whole lines per run)
        pitch = -(-nb // align) * align
        blooms = torch.randint(0, 256, (ncols, pitch), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        check(L.bigsi_hip_insert_columns_device(st.handle, 0, 512, blooms.data_ptr(), pitch))      # warm
        check(L.bigsi_hip_set_profiling(st.handle, 1))
        stats(st)
        check(L.bigsi_hip_insert_columns_device(st.handle, 0, ncols, blooms.data_ptr(), pitch))
        s = stats(st)
        check(L.bigsi_hip_set_profiling(st.handle, 0))
        moved = 2 * ncols * nb
        st.res.written[:] = True
        for r in (0, 1, 511, 512, m // 2 + 3, m - 1):
            bits = ((blooms[:, r >> 3] >> (7 - (r & 7))) & 1).cpu().numpy()
            assert np.array_equal(st.get_rows_packed([r], (ncols + 7) // 8)[0], np.packbits(bits)), r
        emit("transpose_device", m=m, cols=ncols, kernels_ms=s.transpose_ms, bytes_in_plus_out=moved,
             GBps=moved / s.transpose_ms / 1e6, frac=moved / s.transpose_ms / 1e6 / PEAK, filter_pitch=pitch,
             note="k_transpose_regs (+ k_insert_columns for ragged edges); filters resident in HBM")
        del blooms
        st.delete_all()


def colpop():
    """Sample statistics: the full unmasked sweep of column_popcounts over the C3 index and a C4 shard, and a masked sweep at mask
    density 0.25 (bytes = the selected rows only), beside the box's bare sorted-row stream (bigsi_hip_probe_rows).  Wall-clock
    time of the whole call (scratch allocation, both kernels, the copy of the counts); kernel times come from the same command
    under `rocprofv3 --kernel-trace --stats`.  BIGSI_COLPOP_SHAPES="MxN,..." replaces the two shapes."""
    L = _lib.lib()
    shapes = ((10_000_000, 100_000, 4), (25_000_000, 62_500, 3))
    if os.environ.get("BIGSI_COLPOP_SHAPES"):
        shapes = tuple(tuple(int(x) for x in sh.split("x")) + (3,) for sh in os.environ["BIGSI_COLPOP_SHAPES"].split(","))
    for m, n, h in shapes:
        st, fill = open_index("colpop", m, n, h)
        stride = int(st.res.info().row_stride_bytes)
        g_, m_ = _lib.C.c_double(0), _lib.C.c_double(0)
        check(L.bigsi_hip_probe_rows(st.handle, 3880, 1, 1, 0, 3, _lib.C.byref(g_), _lib.C.byref(m_)))
        rng = np.random.default_rng(5)
        sel = rng.random(m) < 0.25
        mask = np.packbits(sel)
        for name, mk, rows in (("unmasked", None, m), ("masked_0.25", mask, int(sel.sum()))):
            counts = st.column_popcounts(mk)               # warm
            reps, ts = 5, []
            for _ in range(reps):
                t0 = time.perf_counter()
                counts = st.column_popcounts(mk)
                ts.append((time.perf_counter() - t0) * 1e3)
            call = sorted(ts)[reps // 2]
            emit("column_popcounts_" + name, m=m, cols=n, stride_bytes=stride, rows_read=rows, bytes=rows * stride, call_ms=call,
                 call_GBps=rows * stride / call / 1e6, box_sorted_GBps=g_.value, counts_sum=int(counts.sum()), counts_max=int(counts.max()),
                 note="fill %.2f s; median of %d calls, wall clock (allocation + k_col_popcount + k_col_popcount_sum + D2H)" % (fill, reps))
        st.delete_all()


def compact():
    """Column compaction (k_compact_columns) on the C3 index and a C4 shard at keep densities 0.99 (a vacuum), 0.5 and 0.1 (an
    extraction), in place and out of place, beside two yardsticks from the same box: the bare sorted-row stream
    (bigsi_hip_probe_rows) and a bigsi_hip_reserve_cols re-stride of the same matrix -- a pure copy of the same rows, what compaction
    would cost if the bit work were free.  bytes = the source words read + the destination stride written (the kernel zeroes the
    row up to its stride).  Wall-clock time of the whole C call: compaction includes its table upload, an extraction goes into a
    destination reserved beforehand, the re-stride includes the allocation of the copy and the release of the old matrix (the
    `copy_all_kept` line is the same copy through k_compact_columns without either: an extraction that keeps every column).
    What does not fit beside the index in device memory is skipped and says so."""
    import torch
    L, C = _lib.lib(), _lib.C
    shapes = ((10_000_000, 100_000), (25_000_000, 62_500))

    for m, n in shapes:
        st, fill = open_index("compact", m, n, 3)
        stride = int(st.res.info().row_stride_bytes)
        src_bytes = m * (-(-n // 64)) * 8
        g_, m_ = C.c_double(0), C.c_double(0)
        check(L.bigsi_hip_probe_rows(st.handle, 3880, 1, 1, 0, 3, C.byref(g_), C.byref(m_)))
        rng = np.random.default_rng(9)
        common = dict(m=m, cols=n, stride_bytes=stride, box_sorted_GBps=g_.value)
        results = {}
        for density in (0.99, 0.5, 0.1):
            flags = rng.random(n) < density
            keep, k = np.ascontiguousarray(np.packbits(flags)), int(flags.sum())
            # out of place, into a destination that already has its capacity
            need = m * stride_for(k)
            free = torch.cuda.mem_get_info()[0]
            if need + (2 << 30) > free:
                emit("compact_extract", density=density, kept=k, skipped="the destination (%d bytes) does not fit beside the index (%d free)" % (need, free), **common)
            else:
                dst = C.c_void_p()
                check(L.bigsi_hip_open(m, 0, k, 3, 0, C.byref(dst)))
                ms = timed(lambda: L.bigsi_hip_extract_columns(dst, st.handle, _lib.ptr(keep)))
                moved = src_bytes + need
                emit("compact_extract", density=density, kept=k, call_ms=ms, bytes=moved, GBps=moved / ms / 1e6, **common)
                results[("extract", density)] = ms
                check(L.bigsi_hip_close(dst))
            # in place; then the index gets its width and its contents back
            ms = timed(lambda: L.bigsi_hip_compact_columns(st.handle, _lib.ptr(keep), None))
            moved = src_bytes + m * stride
            emit("compact_in_place", density=density, kept=k, call_ms=ms, bytes=moved, GBps=moved / ms / 1e6, **common)
            results[("in_place", density)] = ms
            check(L.bigsi_hip_set_num_cols(st.handle, n))
            st.fill_synthetic(SEED, 0, 2)
        # the copy of every column through k_compact_columns (all masks all ones), then the re-stride: the yardstick
        free = torch.cuda.mem_get_info()[0]
        if m * stride + (2 << 30) > free:
            emit("compact_restride_yardstick", skipped="a second copy of the matrix (%d bytes) does not fit beside it (%d free)" % (m * stride, free), **common)
        else:
            dst = C.c_void_p()
            check(L.bigsi_hip_open(m, 0, n, 3, 0, C.byref(dst)))
            every = np.full((n + 7) // 8, 0xFF, np.uint8)
            ms = timed(lambda: L.bigsi_hip_extract_columns(dst, st.handle, _lib.ptr(every)))
            emit("compact_copy_all_kept", call_ms=ms, bytes=src_bytes + m * stride, GBps=(src_bytes + m * stride) / ms / 1e6, **common)
            check(L.bigsi_hip_close(dst))
            ms = timed(lambda: L.bigsi_hip_reserve_cols(st.handle, stride * 8 + 1))
            new_stride = int(st.res.info().row_stride_bytes)
            # the call allocates the copy and frees the old matrix around k_restride: the same allocation and release, timed alone,
            # are taken off, and the ratios are against what is left -- the copy
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            block = torch.cuda.caching_allocator_alloc(m * new_stride)
            torch.cuda.caching_allocator_delete(block)
            torch.cuda.empty_cache()
            torch.cuda.synchronize()
            alloc_ms = (time.perf_counter() - t0) * 1e3
            copy_ms = ms - alloc_ms
            moved = m * (stride + new_stride)
            emit("compact_restride_yardstick", call_ms=ms, alloc_free_ms=alloc_ms, copy_ms=copy_ms, bytes=moved, GBps=moved / copy_ms / 1e6,
                 new_stride_bytes=new_stride, in_place_099_over_copy=results[("in_place", 0.99)] / copy_ms,
                 extract_099_over_copy=(results[("extract", 0.99)] / copy_ms) if ("extract", 0.99) in results else None,
                 note="bigsi_hip_reserve_cols by one more 128-byte line per row = hipMalloc + k_restride + hipFree; copy_ms = the call less an "
                      "allocation and release of the same size timed alone (k_restride's own time: the same command under rocprofv3 --kernel-trace --stats)",
                 **common)
        st.delete_all()


def fold():
    """Row folding (k_fold_rows) on the C3 index -- by 2 out of place, by 2 in place, by 8 in place -- and on a C4 shard (by 2 in place
    only: a second matrix does not fit beside 198 GB), beside two yardsticks from the same run on the same box: the bare sorted-row
    stream (bigsi_hip_probe_rows) and a bigsi_hip_reserve_cols re-stride of the same matrix, k_restride's pure copy.  bytes = what the
    kernel reads (factor x m' rows, the 16-byte pieces that carry columns) + what it writes (m' rows at the destination stride);
    wall-clock time of the whole C call.  Before every fold the source rows of 64 seeded destination rows are fetched with get_rows,
    and afterwards the folded rows are checked against their OR: the only place the 64-bit row arithmetic meets a real size.  What
    does not fit beside the index in device memory is skipped and says so.  BIGSI_FOLD_SHAPES="MxN,..." replaces the two shapes (the
    first runs everything, the others the in-place fold by 2)."""
    import torch
    L, C = _lib.lib(), _lib.C
    shapes = ((10_000_000, 100_000), (25_000_000, 62_500))
    if os.environ.get("BIGSI_FOLD_SHAPES"):
        shapes = tuple(tuple(int(x) for x in sh.split("x")) for sh in os.environ["BIGSI_FOLD_SHAPES"].split(","))

    def expectation(handle, m, n, d, seed):
        """(64 seeded destination rows -- the first, the last and one either side of 2^32 words among them --, the OR of their sources)"""
        new_m, stride = m // d, int(info(handle).row_stride_bytes)
        rng = np.random.default_rng(seed)
        edge = (1 << 32) // (stride // 8)                      # the row whose first word is word 2^32 of the matrix
        picks = [0, new_m - 1] + [r % new_m for r in (edge - 1, edge, edge + 1)] + [int(x) for x in rng.integers(0, new_m, 59)]
        dst = np.unique(np.array(picks, np.uint64))
        src = (dst[None, :] + (np.arange(d, dtype=np.uint64) * np.uint64(new_m))[:, None]).reshape(-1)
        rows = get_rows(handle, src, stride).reshape(d, dst.size, stride)
        want = np.bitwise_or.reduce(rows, axis=0)
        bits = np.unpackbits(want, axis=1)
        bits[:, n:] = 0
        return dst, np.packbits(bits, axis=1)

    def info(handle):
        inf = _lib.Info()
        check(L.bigsi_hip_get_info(handle, C.byref(inf)))
        return inf

    def moved_bytes(m, n, d, dst_stride):
        return m * (-(-(-(-n // 64)) // 2) * 2) * 8 + (m // d) * dst_stride

    for si, (m, n) in enumerate(shapes):
        st, fill = open_index("fold", m, n, 3)
        stride = int(st.res.info().row_stride_bytes)
        g_, m_ = C.c_double(0), C.c_double(0)
        check(L.bigsi_hip_probe_rows(st.handle, 3880, 1, 1, 0, 3, C.byref(g_), C.byref(m_)))
        common = dict(m=m, cols=n, stride_bytes=stride, box_sorted_GBps=g_.value, lib=os.path.basename(_lib.LIB_PATH))
        results = {}
        if si == 0:
            # out of place by 2, into a destination that already has its capacity
            need = (m // 2) * stride
            free = torch.cuda.mem_get_info()[0]
            if need + (2 << 30) > free:
                emit("fold_into", factor=2, skipped="the destination (%d bytes) does not fit beside the index (%d free)" % (need, free), **common)
            else:
                ids, want = expectation(st.handle, m, n, 2, 1)
                dst = C.c_void_p()
                check(L.bigsi_hip_open(m // 2, 0, n, 3, 0, C.byref(dst)))
                ms = timed(lambda: L.bigsi_hip_fold_rows_into(dst, st.handle))
                ok = bool(np.array_equal(get_rows(dst, ids, stride), want))
                moved = moved_bytes(m, n, 2, int(info(dst).row_stride_bytes))
                emit("fold_into", factor=2, call_ms=ms, bytes=moved, GBps=moved / ms / 1e6, rows_checked=int(ids.size), rows_ok=ok, **common)
                results["into2"] = moved / ms
                check(L.bigsi_hip_close(dst))
                assert ok
        for d in ((2, 8) if si == 0 else (2,)):
            if m % d:
                emit("fold_in_place", factor=d, skipped="%d does not divide %d" % (d, m), **common)
                continue
            ids, want = expectation(st.handle, m, n, d, 2 + d)
            ms = timed(lambda: L.bigsi_hip_fold_rows(st.handle, d, None))
            ok = bool(np.array_equal(get_rows(st.handle, ids, stride), want)) and int(info(st.handle).num_rows) == m // d
            moved = moved_bytes(m, n, d, stride)
            emit("fold_in_place", factor=d, call_ms=ms, bytes=moved, GBps=moved / ms / 1e6, rows_checked=int(ids.size), rows_ok=ok, **common)
            results["in_place%d" % d] = moved / ms
            assert ok
            st.delete_all()                                    # (the index has m / d rows now: a fresh one for what follows)
            st, fill = open_index("fold", m, n, 3)
        # the yardstick: a re-stride of the same matrix, a pure copy of the same rows
        free = torch.cuda.mem_get_info()[0]
        if m * (stride + 128) + (2 << 30) > free:
            emit("fold_restride_yardstick", skipped="a second copy of the matrix (%d bytes) does not fit beside it (%d free)" % (m * (stride + 128), free),
                 fold_by_2_in_place_over_box=results["in_place2"] / 1e6 / g_.value if "in_place2" in results else None, **common)
        else:
            ms = timed(lambda: L.bigsi_hip_reserve_cols(st.handle, stride * 8 + 1))
            new_stride = int(st.res.info().row_stride_bytes)
            # The call is hipMalloc + k_restride + hipFree, and for 125 GB the two runtime calls take seconds where the kernel takes
            # tens of milliseconds.  Both are timed alone here, through the very runtime the library calls (the same hipMalloc /
            # hipFree, the same size), and BOTH figures are printed: call_ms is what was measured, call_less_alloc_ms is the
            # difference of two terms of seconds and carries their noise (it can come out negative).  k_restride's own time is the
            # kernel trace's: this command under `rocprofv3 --kernel-trace --stats`, where k_fold_rows' times stand beside it.
            hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64.so" in line))
            block = C.c_void_p()
            t0 = time.perf_counter()
            assert hip.hipMalloc(C.byref(block), C.c_size_t(m * new_stride)) == 0
            assert hip.hipFree(block) == 0
            alloc_ms = (time.perf_counter() - t0) * 1e3
            moved = m * (stride + new_stride)
            emit("fold_restride_yardstick", call_ms=ms, alloc_free_ms=alloc_ms, call_less_alloc_ms=ms - alloc_ms, bytes=moved, new_stride_bytes=new_stride,
                 fold_GBps={k: v / 1e6 for k, v in results.items()},
                 **{"fold_%s_rate_over_box" % k: v / 1e6 / g_.value for k, v in results.items()},
                 note="bigsi_hip_reserve_cols by one more 128-byte line per row = hipMalloc + k_restride + hipFree; alloc_free_ms = a hipMalloc + hipFree "
                      "of the new matrix's size timed alone through the same runtime; call_less_alloc_ms is NOT a kernel time (a difference of two "
                      "terms of seconds); k_restride's copy time: the kernel trace of this command (rocprofv3 --kernel-trace --stats)",
                 **common)
        st.delete_all()


def prevalence():
    """K-mer prevalence (bigsi_hip_kmer_prevalence): one 1 kbp query and 8192 x 1 kbp on the C3 index, 256 x 1 kbp on a C4 shard.
    Per workload: the sweep's algorithmic bytes (unique k-mers x h x ceil(N / 64) x 8), the sweep by the library's HIP events on the
    index stream (k_kmer_prevalence + k_kmer_prevalence_sum: presence_ms of bigsi_hip_stats), the exact run in front of it (K1 +
    row-AND + K4), the whole call by the wall clock, and the box's bare random-row and sorted-row streams of the same run
    (bigsi_hip_probe_rows).  The yardstick is the RANDOM-row rate: a k-mer's h rows meet in one lane, so the list cannot be
    address-ordered.  On the first shape, 64 k-mers -- three of them with a row next to the one whose word offset passes 2^32 -- are
    checked against the popcounts of bigsi_hip_lookup's rows.  BIGSI_PREVALENCE_SHAPES="MxNxHxQ,..." replaces the workloads."""
    L, C = _lib.lib(), _lib.C
    work = ((10_000_000, 100_000, 4, (1, 8192)), (25_000_000, 62_500, 3, (256,)))
    if os.environ.get("BIGSI_PREVALENCE_SHAPES"):
        work = tuple((int(a), int(b), int(c), (int(d),)) for a, b, c, d in (sh.split("x") for sh in os.environ["BIGSI_PREVALENCE_SHAPES"].split(",")))
    first = True
    for m, n, h, sizes in work:
        st, fill = open_index("prevalence", m, n, h)
        wv = -(-n // 64)
        box = {}
        for name, srt in (("box_random_GBps", 0), ("box_sorted_GBps", 1)):
            g_, m_ = C.c_double(0), C.c_double(0)
            check(L.bigsi_hip_probe_rows(st.handle, 3880, 1, srt, 0, 3, C.byref(g_), C.byref(m_)))
            box[name] = g_.value
        rng = np.random.default_rng(11)
        for q in sizes:
            seqs = rand_seqs(rng, q, 1000)
            unique = sum(len({s[i:i + 31] for i in range(970)}) for s in seqs)
            ab = unique * h * wv * 8
            reps = 3 if ab < 50e9 else 1
            if reps > 1:
                st.kmer_prevalence(seqs, 31)            # warm (a single pass of hundreds of GB is its own steady state)
            check(L.bigsi_hip_set_profiling(st.handle, 1))
            stats(st)
            t0 = time.perf_counter()
            for _ in range(reps):
                pos, total, _ = st.kmer_prevalence(seqs, 31)
            call = (time.perf_counter() - t0) / reps * 1e3
            s_ = stats(st)
            check(L.bigsi_hip_set_profiling(st.handle, 0))
            sweep = s_.presence_ms / reps
            emit("kmer_prevalence", m=m, cols=n, h=h, n_seqs=q, unique_kmers=unique, alg_bytes=ab, sweep_ms=sweep, sweep_GBps=ab / sweep / 1e6,
                 sweep_over_box_random=ab / sweep / 1e6 / box["box_random_GBps"], exact_run_ms=(s_.and_ms + s_.kmerize_ms + s_.compact_ms) / reps,
                 call_ms=call, total_sum=int(total.sum(dtype=np.uint64)), total_max=int(total.max()),
                 note="fill %.2f s; mean of %d call(s); sweep = both kernels by HIP events, exact run = K1 + row-AND + K4 by HIP events" % (fill, reps), **box)
        if first:
            first = False
            # k-mers with a row id next to the row where row x stride_words passes 2^32 words: K1 on a narrow index of the same m finds them
            stride_words = int(st.res.info().row_stride_bytes) // 8
            edge = (1 << 32) // stride_words
            hits = {}          # row id -> the text of a k-mer that has it
            if edge + 1 < m:
                small, _ = open_index("prevalence_ids", m, 64, h)
                for _ in range(16):
                    long_seqs = rand_seqs(rng, 4096, 1000)
                    b = small.new_batch(long_seqs, 31)
                    b.run(1.0)
                    _, nu, _ = b.unique()
                    for i, s in enumerate(long_seqs):
                        rows = b.rows(i, nu[i])
                        for r in (edge - 1, edge, edge + 1):
                            j = np.flatnonzero((rows == r).any(axis=1))
                            if len(j) and r not in hits:
                                seen, order = set(), []          # unique k-mer j[0] of the sequence, in first-occurrence order
                                for p in range(len(s) - 30):
                                    if s[p:p + 31] not in seen:
                                        seen.add(s[p:p + 31])
                                        order.append(p)
                                hits[r] = s[order[int(j[0])]:order[int(j[0])] + 31]
                    b.close()
                    if len(hits) == 3:
                        break
                small.delete_all()
            kmers = list(hits.values()) + rand_seqs(rng, 64 - len(hits), 31)
            pos, total, _ = st.kmer_prevalence(kmers, 31)
            rb = (n + 7) // 8
            out = np.zeros((len(kmers), rb), np.uint8)
            check(L.bigsi_hip_lookup(st.handle, "".join(kmers).encode(), 31, len(kmers), _lib.ptr(out)))
            if n % 8:
                out[:, -1] &= (0xFF00 >> (n % 8)) & 0xFF
            want = np.unpackbits(out, axis=1).sum(axis=1, dtype=np.uint64)
            emit("kmer_prevalence_vs_lookup", m=m, cols=n, kmers=len(kmers), edge_row=edge, edge_rows_found=sorted(int(r) for r in hits),
                 equal=bool(np.array_equal(want, total.astype(np.uint64))), total_min=int(total.min()), total_max=int(total.max()))
        st.delete_all()


def collapse():
    """Column collapse (k_collapse_columns) on the C3 index: (a) the identity map, (b) 100 000 -> 1000 groups at random, (c) a
    dereplication -- 1 % of the columns merged in pairs, the rest singletons -- beside two figures from the same run: an extraction that
    keeps every column (the same copy through k_compact_columns) and the bare sorted-row stream (bigsi_hip_probe_rows).  Wall-clock
    time of the whole C call (table upload included) into a destination reserved beforehand; bytes = the source words read + the
    destination stride written; bits = the set bits of the columns that move (bigsi_hip_column_popcounts).  Before each call 64 seeded
    rows are fetched -- the rows either side of row 2 739 137, where row x stride_words passes 2^32, among them -- and checked against
    numpy afterwards.  What does not fit beside the index in device memory is skipped and says so."""
    import torch
    L, C = _lib.lib(), _lib.C
    m, n = 10_000_000, 100_000
    DROPPED = 0xFFFFFFFF

    st, fill = open_index("collapse", m, n, 3)
    stride = int(st.res.info().row_stride_bytes)
    src_bytes = m * (-(-n // 64)) * 8
    g_, m_ = C.c_double(0), C.c_double(0)
    check(L.bigsi_hip_probe_rows(st.handle, 3880, 1, 1, 0, 3, C.byref(g_), C.byref(m_)))
    counts = np.zeros(n, np.uint64)
    check(L.bigsi_hip_column_popcounts(st.handle, None, _lib.ptr(counts), n))
    rng = np.random.default_rng(10)
    edge = (1 << 32) // (stride // 8)          # the first row whose offset in words is >= 2^32
    ids = np.unique(np.concatenate([rng.integers(0, m, 61).astype(np.uint64), np.array([edge - 1, edge, edge + 1], np.uint64)]))
    before = np.unpackbits(get_rows(st.handle, ids, (n + 7) // 8), axis=1)[:, :n]
    common = dict(m=m, cols=n, stride_bytes=stride, box_sorted_GBps=g_.value, fill_density=float(counts.sum()) / (m * n), edge_row=int(edge))
    # the yardstick of the same run: the copy of every column through k_compact_columns
    copy_ms = None
    free = torch.cuda.mem_get_info()[0]
    if m * stride + (2 << 30) > free:
        emit("collapse_copy_all_kept_yardstick", skipped="a second copy of the matrix (%d bytes) does not fit beside it (%d free)" % (m * stride, free), **common)
    else:
        dst = C.c_void_p()
        check(L.bigsi_hip_open(m, 0, n, 3, 0, C.byref(dst)))
        every = np.full((n + 7) // 8, 0xFF, np.uint8)
        copy_ms = timed(lambda: L.bigsi_hip_extract_columns(dst, st.handle, _lib.ptr(every)))
        emit("collapse_copy_all_kept_yardstick", call_ms=copy_ms, bytes=src_bytes + m * stride, GBps=(src_bytes + m * stride) / copy_ms / 1e6, **common)
        check(L.bigsi_hip_close(dst))
    identity = np.arange(n, dtype=np.uint32)
    thousand = rng.integers(0, 1000, n).astype(np.uint32)
    derep = np.zeros(n, np.uint32)
    pairs = rng.choice(n, 1000, replace=False)          # 1 % of the columns, merged in pairs: the second of a pair takes the first's group
    second = np.zeros(n, bool)
    second[pairs[1::2]] = True
    derep[~second] = np.arange(int((~second).sum()), dtype=np.uint32)
    derep[pairs[1::2]] = derep[pairs[0::2]]
    for name, group_of, groups in (("identity", identity, n), ("random_1000", thousand, 1000), ("dereplicate_1pct", derep, int((~second).sum()))):
        need = m * stride_for(groups)
        free = torch.cuda.mem_get_info()[0]
        if need + (2 << 30) > free:
            emit("collapse_" + name, groups=groups, skipped="the destination (%d bytes) does not fit beside the index (%d free)" % (need, free), **common)
            continue
        dst = C.c_void_p()
        check(L.bigsi_hip_open(m, 0, groups, 3, 0, C.byref(dst)))
        ms = timed(lambda: L.bigsi_hip_collapse_columns_into(dst, st.handle, _lib.ptr(group_of), groups))
        want = np.zeros((groups, ids.size), np.uint8)
        cols = np.flatnonzero(group_of != DROPPED)
        np.maximum.at(want, group_of[cols].astype(np.int64), before[:, cols].T)
        got = get_rows(dst, ids, need // m)
        exp = np.zeros_like(got)
        packed = np.packbits(want.T, axis=1)
        exp[:, :packed.shape[1]] = packed
        bits = int(counts[cols].sum())
        emit("collapse_" + name, groups=groups, call_ms=ms, bytes=src_bytes + need, GBps=(src_bytes + need) / ms / 1e6, bits_moved=bits,
             Gbits_per_s=bits / ms / 1e6, over_copy_all_kept=(ms / copy_ms) if copy_ms else None, rows_checked=int(ids.size),
             rows_equal=bool(np.array_equal(got, exp)), source_unchanged=bool(np.array_equal(np.unpackbits(get_rows(st.handle, ids, (n + 7) // 8), axis=1)[:, :n], before)),
             **common)
        check(L.bigsi_hip_close(dst))
    st.delete_all()


def consensus():
    """Consensus collapse (k_consensus_columns) on the C3 index beside the OR collapse of the SAME RUN on the same map: the collapse's
    workload (b), 100 000 -> 1000 groups at random, with every group asking for 1 member, 50 % and 100 % of its size, and its
    workload (c), the dereplication map (pairs and singletons), at 100 %.  Wall-clock time of the whole C call (table upload
    included) into a destination reserved beforehand, each as a ratio over bigsi_hip_collapse_columns_into.  64 seeded rows -- the
    rows either side of the one where row x stride_words passes 2^32 among them -- are checked against numpy after each call.  What
    does not fit beside the index in device memory is skipped and says so."""
    import torch
    from bigsi_amd.consensus import group_sizes, need_of
    L, C = _lib.lib(), _lib.C
    m, n = 10_000_000, 100_000

    st, fill = open_index("consensus", m, n, 3)
    stride = int(st.res.info().row_stride_bytes)
    src_bytes = m * (-(-n // 64)) * 8
    counts = np.zeros(n, np.uint64)
    check(L.bigsi_hip_column_popcounts(st.handle, None, _lib.ptr(counts), n))
    rng = np.random.default_rng(10)
    edge = (1 << 32) // (stride // 8)          # the first row whose offset in words is >= 2^32
    ids = np.unique(np.concatenate([rng.integers(0, m, 61).astype(np.uint64), np.array([edge - 1, edge, edge + 1], np.uint64)]))
    before = np.unpackbits(get_rows(st.handle, ids, (n + 7) // 8), axis=1)[:, :n].astype(np.int64)
    common = dict(m=m, cols=n, stride_bytes=stride, fill_density=float(counts.sum()) / (m * n), edge_row=int(edge))
    thousand = rng.integers(0, 1000, n).astype(np.uint32)          # (the same draws as collapse(): the same two maps)
    derep = np.zeros(n, np.uint32)
    pairs = rng.choice(n, 1000, replace=False)
    second = np.zeros(n, bool)
    second[pairs[1::2]] = True
    derep[~second] = np.arange(int((~second).sum()), dtype=np.uint32)
    derep[pairs[1::2]] = derep[pairs[0::2]]
    for name, group_of, groups, percents in (("random_1000", thousand, 1000, (1, 50, 100)), ("dereplicate_1pct", derep, int((~second).sum()), (100,))):
        room = m * stride_for(groups)
        free = torch.cuda.mem_get_info()[0]
        if room + (2 << 30) > free:
            emit("consensus_" + name, groups=groups, skipped="the destination (%d bytes) does not fit beside the index (%d free)" % (room, free), **common)
            continue
        sizes = group_sizes(group_of, groups)
        order = np.argsort(group_of, kind="stable")          # (every column has a group in both maps) the sampled rows' member counts:
        starts = np.flatnonzero(np.r_[True, np.diff(group_of[order].astype(np.int64)) != 0])
        have = np.zeros((ids.size, groups), np.int64)
        have[:, group_of[order][starts]] = np.add.reduceat(before[:, order], starts, axis=1)
        dst = C.c_void_p()
        check(L.bigsi_hip_open(m, 0, groups, 3, 0, C.byref(dst)))
        or_ms = timed(lambda: L.bigsi_hip_collapse_columns_into(dst, st.handle, _lib.ptr(group_of), groups))
        check(L.bigsi_hip_close(dst))
        emit("consensus_%s_or_collapse_yardstick" % name, groups=groups, call_ms=or_ms, bytes=src_bytes + room, bits_moved=int(counts.sum()), **common)
        for percent in percents:
            need = need_of(sizes, percent) if percent > 1 else np.ones(groups, np.uint32)
            dst = C.c_void_p()
            check(L.bigsi_hip_open(m, 0, groups, 3, 0, C.byref(dst)))
            ms = timed(lambda: L.bigsi_hip_consensus_columns_into(dst, st.handle, _lib.ptr(group_of), groups, _lib.ptr(need)))
            got = get_rows(dst, ids, room // m)
            exp = np.zeros_like(got)
            packed = np.packbits(have >= need.astype(np.int64)[None, :], axis=1)
            exp[:, :packed.shape[1]] = packed
            emit("consensus_%s_need_%s" % (name, "1" if percent == 1 else "%dpct" % percent), groups=groups, largest_group=int(sizes.max()),
                 field_bits=8 if sizes.max() <= 255 else 16 if sizes.max() <= 65535 else 32, call_ms=ms, or_collapse_ms=or_ms, over_or_collapse=ms / or_ms,
                 bytes=src_bytes + room, bits_counted=int(counts.sum()), Gbits_per_s=float(counts.sum()) / ms / 1e6, fill_out_sampled=float(np.unpackbits(got, axis=1)[:, :groups].mean()),
                 rows_checked=int(ids.size), rows_equal=bool(np.array_equal(got, exp)), **common)
            check(L.bigsi_hip_close(dst))
    st.delete_all()


# the VALU rate the pairwise bound is derived from: CUs x SIMDs x lanes per clock x clock of the MI355X data sheet, NOT measured here
PAIR_VALU_LANES_PER_CLOCK = 256 * 4 * 32
PAIR_CLOCK_HZ = 2.4e9


def pairwise():
    """Pairwise popcounts (k_columns_to_planes, k_pair_popcount, k_pair_popcount_sum) on the C3 index at the collapse workload's
    density: symmetric S = 1024 and S = 4096 (columns spread evenly over the width) and one rectangular 64 x 16384, beside two
    figures of the same run: one unmasked column_popcounts sweep (the time of reading the matrix once: phase 1's yardstick when
    the selection touches every line) and the route that exists today, a masked column_popcounts per sample (get_column + the masked
    sweep, timed for 8 of the columns and scaled to S).  Wall-clock time of the whole C call, and the kernel times of the three phases
    from a second, profiled call (HIP events, the call waits after every launch; the per-kernel table: this command under
    `rocprofv3 --kernel-trace --stats`).  Phase 2's rate in pair-words/s (a pair-word: 64 rows of one pair, 4 VALU operations)
    stands beside the bound 4 operations per pair-word give at the data sheet's lane count and clock (not measured here).  A sample
    of the counts is checked against rows fetched from the index."""
    L, C = _lib.lib(), _lib.C
    m, n = 10_000_000, 100_000
    st, fill = open_index("pairwise", m, n, 3)
    stride = int(st.res.info().row_stride_bytes)
    counts = st.column_popcounts()          # warm
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        counts = st.column_popcounts()
        ts.append((time.perf_counter() - t0) * 1e3)
    sweep_ms = sorted(ts)[1]
    common = dict(m=m, cols=n, stride_bytes=stride, fill_density=float(counts.sum()) / (m * n), unmasked_sweep_ms=sweep_ms,
                  unmasked_sweep_GBps=m * stride / sweep_ms / 1e6)
    emit("pairwise_unmasked_sweep_yardstick", call_ms=sweep_ms, bytes=m * stride, note="fill %.2f s; median of 3 calls, wall clock" % fill, **common)
    # the route that exists today: per sample its column as a row mask, then the masked sweep of every column
    rng = np.random.default_rng(11)
    eight = rng.choice(n, 8, replace=False)
    st.column_popcounts(np.frombuffer(st.get_column(int(eight[0])), np.uint8))          # warm
    t0 = time.perf_counter()
    for c in eight:
        st.column_popcounts(np.frombuffer(st.get_column(int(c)), np.uint8))
    per_sample_ms = (time.perf_counter() - t0) * 1e3 / 8
    emit("pairwise_today_masked_sweep_per_sample", call_ms=per_sample_ms, samples_timed=8, **common)
    bound = PAIR_VALU_LANES_PER_CLOCK * PAIR_CLOCK_HZ / 4
    ids = np.unique(rng.integers(0, m, 4096).astype(np.uint64))
    rows = np.unpackbits(get_rows(st.handle, ids, (n + 7) // 8), axis=1)[:, :n]
    shapes = (("symmetric_1024", np.linspace(0, n - 1, 1024).astype(np.uint32), None),
              ("symmetric_4096", np.linspace(0, n - 1, 4096).astype(np.uint32), None),
              ("rect_64x16384", np.linspace(0, n - 1, 64).astype(np.uint32), np.linspace(3, n - 4, 16384).astype(np.uint32)))
    for name, a, b in shapes:
        na, nb = a.size, a.size if b is None else b.size
        out = np.zeros((na, nb), np.uint64)
        call = lambda: L.bigsi_hip_pairwise_popcounts(st.handle, _lib.ptr(a), na, _lib.ptr(b), 0 if b is None else nb, _lib.ptr(out), out.size)  # noqa: E731
        check(call())          # warm
        ms = min(timed(call), timed(call))
        check(L.bigsi_hip_set_profiling(st.handle, 1))
        check(call())
        phase = (C.c_double * 4)()
        check(L.bigsi_hip_pairwise_phase_ms(st.handle, phase))
        check(L.bigsi_hip_set_profiling(st.handle, 0))
        distinct = np.unique(a).size if b is None else np.unique(np.concatenate([a, b])).size
        words = np.unique((a if b is None else np.concatenate([a, b])) // 64).size
        tiles_a, tiles_b = -(-np.unique(a).size // 64), -(-(np.unique(a).size if b is None else np.unique(b).size) // 64)
        tiles = tiles_a * (tiles_a + 1) // 2 if b is None else tiles_a * tiles_b
        pair_words = tiles * 64 * 64 * (-(-m // 64))          # what the kernel computes: whole tiles, the upper triangle when symmetric
        # checks: the diagonal against column_popcounts and the symmetry (exact); 64 pairs against 4096 fetched rows (a subset of
        # the rows: a lower bound); one row against today's route, the masked sweep under that sample's column (exact)
        ok = None
        if b is None:
            ok = bool(np.array_equal(out.diagonal(), counts[a]) and np.array_equal(out, out.T))
        sample_ok = bool((rows[:, a[:8]].T.astype(np.uint64) @ rows[:, (a if b is None else b)[:8]].astype(np.uint64) <= out[:8, :8]).all())
        masked_check = None
        if b is None:          # one column of today's route against the same column here
            c0 = int(a[5])
            mk = st.column_popcounts(np.frombuffer(st.get_column(c0), np.uint8))
            masked_check = bool(np.array_equal(mk[a], out[5]))
        emit("pairwise_" + name, na=na, nb=nb, distinct_columns=int(distinct), source_words=int(words), call_ms=ms, chunks=int(phase[3]),
             planes_ms=phase[0], pairs_ms=phase[1], sum_ms=phase[2], planes_over_unmasked_sweep=phase[0] / sweep_ms,
             pair_words=int(pair_words), pair_words_per_s=pair_words / phase[1] * 1e3, derived_bound_pair_words_per_s=bound,
             frac_of_derived_bound=pair_words / phase[1] * 1e3 / bound,
             bound_note="4 VALU ops per pair-word at %d lanes/clock x %.1f GHz: data sheet, not measured here" % (PAIR_VALU_LANES_PER_CLOCK, PAIR_CLOCK_HZ / 1e9),
             today_ms_scaled=per_sample_ms * na, today_over_this=per_sample_ms * na / ms, diagonal_and_symmetry_ok=ok, sampled_rows_lower_bound_ok=sample_ok,
             equals_masked_sweep_of_one_column=masked_check, **common)
    st.delete_all()


def tally():
    """Query-set tally (bigsi_hip_tally_add_stream) beside bigsi_hip_search_stream on the same input in the same run: 8192 x 1 kbp on
    the C3 index (10 M x 100 k, h = 4), hit-sparse as drawn and hit-dense (bench.py's c5_dense recipe: every 16th query held whole by
    1 % of the samples), at threshold 1.0 and 0.4; 65 536 reads of 61 bp on BASELINE configs[1]'s index (1 M x 10 k, h = 3), where the
    search stream takes the one-launch read kernel and the tally cannot.  Per line: wall ms of one call of each (best of 3 after a
    warm call; the tally's includes its reset and fetch), the tally kernels' own time (HIP events around k_tally_hits +
    k_tally_totals: compact_ms of bigsi_hip_stats under profiling level 1, a run of its own) beside that run's row-AND and K1 time,
    the time numpy takes from the search stream's hit lists to the same two vectors (two bincounts), and whether the vectors agree."""
    L = _lib.lib()

    def line(name, st, n_cols, seqs, thr, note):
        blob, off = _lib.pack_seqs(seqs)
        t = st.new_tally()

        def tally_call():
            t.reset()
            check(L.bigsi_hip_tally_add_stream(t.b, blob, _lib.ptr(off), len(seqs), 31, float(thr)))
            return t.fetch()
        tally_call()
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            got = tally_call()
            walls.append((time.perf_counter() - t0) * 1e3)
        check(L.bigsi_hip_set_profiling(st.handle, 1))
        stats(st)
        tally_call()
        s = stats(st)
        check(L.bigsi_hip_set_profiling(st.handle, 0))
        st.search_many_packed(blob, off, 31, thr)
        search, counted = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            nk, nu, hoff, col, cnt = st.search_many_packed(blob, off, 31, thr)
            t1 = time.perf_counter()
            qh = np.bincount(col, minlength=n_cols).astype(np.uint64)
            kf = np.bincount(col, weights=cnt, minlength=n_cols).astype(np.uint64)          # (float64 sums of integers below 2^53: exact)
            t2 = time.perf_counter()
            search.append((t1 - t0) * 1e3)
            counted.append((t2 - t1) * 1e3)
        agree = bool(np.array_equal(qh, got[0]) and np.array_equal(kf, got[1]) and int(got[2][0]) == int((nu > 0).sum()) and int(got[2][1]) == int(nu.sum()))
        step_prof = s.kmerize_ms + s.and_ms + s.compact_ms
        emit(name, threshold=thr, n_seqs=len(seqs), cols=n_cols, hits=int(hoff[-1]), samples_hit=int((got[0] > 0).sum()), queries_with_hits=int(got[2][3]),
             tally_stream_ms=min(walls), search_stream_ms=min(search), bincount_ms=min(counted), search_plus_bincount_ms=min(search) + min(counted),
             tally_kernels_ms=s.compact_ms, row_and_ms=s.and_ms, k1_ms=s.kmerize_ms, tally_kernels_frac_of_device=s.compact_ms / step_prof if step_prof else None,
             tally_kernels_frac_of_call=s.compact_ms / min(walls), agree_with_search=agree, note=note)
        t.close()
        assert agree, name

    m, n, h = 10_000_000, 100_000, 4
    st, _ = open_index("tally", m, n, h)
    rng = np.random.default_rng(11)
    seqs = rand_seqs(rng, 8192, 1000)
    for thr in (1.0, 0.4):
        line("tally_c3_sparse", st, n, seqs, thr, "8192 x 1 kbp as drawn")
    held, cols = seqs[::16], np.sort(rng.choice(n, size=n // 100, replace=False))
    t0 = time.time()
    for c in cols:
        st.insert_kmers(int(c), held, 31)
    plant_s = time.time() - t0
    for thr in (1.0, 0.4):
        line("tally_c3_dense", st, n, seqs, thr, "every 16th query held by 1 %% of the samples (planted in %.1f s)" % plant_s)
    st.delete_all()
    st, _ = open_index("tally_reads", 1_000_000, 10_000, 3)
    reads = rand_seqs(rng, 65536, 61)
    for thr in (1.0, 0.4):
        line("tally_c2_reads", st, 10_000, reads, thr, "65 536 reads of 61 bp: the search stream takes the one-launch read kernel, the tally the non-fused route")
    st.delete_all()


def classify():
    """Read classification (bigsi_hip_classify_stream) beside the query-set tally (bigsi_hip_tally_add_stream + fetch) on the same input
    in the same run -- the tally's inputs: 8192 x 1 kbp on the C3 index (10 M x 100 k, h = 4), hit-sparse as drawn and hit-dense (every
    16th query held whole by 1 % of the samples), at threshold 1.0 and 0.4; 65 536 reads of 61 bp on 1 M x 10 k, h = 3.  group_of: 100
    groups of neighbouring colours.  Per line: wall ms of one call of each (best of 3 after a warm call, the two alternating; the
    tally's includes its reset and fetch), their ratio, and from one profiled call of each (level 1, runs of their own) the kernel's own
    time by HIP events (k_classify_groups, resp. k_tally_hits + k_tally_totals: compact_ms of bigsi_hip_stats) beside that call's
    row-AND and K1 time."""
    L = _lib.lib()
    from bigsi_amd.classify import RECORD_DTYPE

    def line(name, st, n_cols, seqs, thr, note):
        blob, off = _lib.pack_seqs(seqs)
        t = st.new_tally()
        n_groups = 100
        group_of = (np.arange(n_cols, dtype=np.uint64) * n_groups // n_cols).astype(np.uint32)
        records = np.zeros(len(seqs), RECORD_DTYPE)

        def tally_call():
            t.reset()
            check(L.bigsi_hip_tally_add_stream(t.b, blob, _lib.ptr(off), len(seqs), 31, float(thr)))
            return t.fetch()

        def classify_call():
            check(L.bigsi_hip_classify_stream(st.handle, blob, _lib.ptr(off), len(seqs), 31, float(thr), _lib.ptr(group_of), n_cols, n_groups, _lib.ptr(records)))
        tally_call()
        classify_call()
        walls_t, walls_c = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            got = tally_call()
            t1 = time.perf_counter()
            classify_call()
            t2 = time.perf_counter()
            walls_t.append((t1 - t0) * 1e3)
            walls_c.append((t2 - t1) * 1e3)
        check(L.bigsi_hip_set_profiling(st.handle, 1))
        stats(st)
        classify_call()
        sc = stats(st)
        tally_call()
        stl = stats(st)
        check(L.bigsi_hip_set_profiling(st.handle, 0))
        # the two calls saw the same hits: the records' grouped hit columns sum to the tally's queries_hit (every column is in a group)
        agree = int(records["samples_hit"].astype(np.uint64).sum()) == int(got[0].sum()) and int((records["num_unique"] > 0).sum()) == int(got[2][0])
        step_prof = sc.kmerize_ms + sc.and_ms + sc.compact_ms
        emit(name, threshold=thr, n_seqs=len(seqs), cols=n_cols, n_groups=n_groups, queries_with_groups=int((records["groups_hit"] > 0).sum()),
             hit_columns=int(records["samples_hit"].astype(np.uint64).sum()), classify_stream_ms=min(walls_c), tally_stream_ms=min(walls_t),
             classify_over_tally=min(walls_c) / min(walls_t), classify_kernel_ms=sc.compact_ms, classify_row_and_ms=sc.and_ms, classify_k1_ms=sc.kmerize_ms,
             classify_kernel_frac_of_device=sc.compact_ms / step_prof if step_prof else None, classify_kernel_frac_of_call=sc.compact_ms / min(walls_c),
             tally_kernels_ms=stl.compact_ms, tally_row_and_ms=stl.and_ms, tally_k1_ms=stl.kmerize_ms, agree_with_tally=agree, note=note)
        t.close()
        assert agree, name

    m, n, h = 10_000_000, 100_000, 4
    st, _ = open_index("classify", m, n, h)
    rng = np.random.default_rng(11)
    seqs = rand_seqs(rng, 8192, 1000)
    for thr in (1.0, 0.4):
        line("classify_c3_sparse", st, n, seqs, thr, "8192 x 1 kbp as drawn")
    held, cols = seqs[::16], np.sort(rng.choice(n, size=n // 100, replace=False))
    t0 = time.time()
    for c in cols:
        st.insert_kmers(int(c), held, 31)
    plant_s = time.time() - t0
    for thr in (1.0, 0.4):
        line("classify_c3_dense", st, n, seqs, thr, "every 16th query held by 1 %% of the samples (planted in %.1f s)" % plant_s)
    st.delete_all()
    st, _ = open_index("classify_reads", 1_000_000, 10_000, 3)
    reads = rand_seqs(rng, 65536, 61)
    for thr in (1.0, 0.4):
        line("classify_c2_reads", st, 10_000, reads, thr, "65 536 reads of 61 bp")
    st.delete_all()


ASSOCIATE_INPUTS = ("sparse", "dense")
ASSOCIATE_CALLS = ("tally", "tally", "classify2", "classify64", "associate2", "associate64")


def associate():
    """Group association (bigsi_hip_associate_stream) beside the read classification (bigsi_hip_classify_stream) and the query-set
    tally (bigsi_hip_tally_add_stream + fetch), ONE PROCESS PER FIGURE: without BIGSI_ASSOCIATE_FIGURE this leg starts a fresh child
    process of itself for every (input, call) pair, one after the other, and relays their lines; with BIGSI_ASSOCIATE_FIGURE =
    "<input>:<call>" it measures that one.  Inputs, on the C3 index (10 M x 100 k, h = 4), threshold 1.0: "sparse" -- 8192 x 1 kbp as
    drawn, the classify leg's input; "dense" -- 256 x 1 kbp, each held whole by the same random half of the columns (one insert_kmers
    per column, as the dense bench legs plant theirs).  Calls: the tally (twice per input: what two processes of a session differ by),
    the classifier and the association with 2 groups (colour parity) and 64 (colour mod 64).  Per line: wall ms of the call (best of
    3 after a warm call, and all three), and from one profiled call (level 1) the consumer kernels' own time by HIP events
    (k_group_counts, k_classify_groups, k_tally_hits + k_tally_totals: compact_ms of bigsi_hip_stats) beside that call's row-AND and
    K1 time; hit_columns for the lines of an input to be compared."""
    import subprocess
    figure = os.environ.get("BIGSI_ASSOCIATE_FIGURE")
    if not figure:
        for inp in ASSOCIATE_INPUTS:
            for call in ASSOCIATE_CALLS:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "associate"], env=dict(os.environ, BIGSI_ASSOCIATE_FIGURE="%s:%s" % (inp, call)),
                                   capture_output=True, text=True, timeout=600)
                sys.stdout.write(r.stdout)
                sys.stdout.flush()
                if r.returncode != 0:          # nothing more is started on the device behind a process that failed
                    sys.stderr.write(r.stderr[-4000:])
                    raise SystemExit("associate figure %s:%s exited with %d" % (inp, call, r.returncode))
        return
    inp, call = figure.split(":")
    assert inp in ASSOCIATE_INPUTS and call in ASSOCIATE_CALLS, figure
    L = _lib.lib()
    from bigsi_amd.associate import INFO_DTYPE
    from bigsi_amd.classify import RECORD_DTYPE
    m, n, h, k = 10_000_000, 100_000, 4, 31
    st, fill_s = open_index("associate", m, n, h)
    rng = np.random.default_rng(11)
    seqs = rand_seqs(rng, 8192, 1000)
    plant_s = 0.0
    if inp == "dense":
        seqs = seqs[:256]
        blob, off = _lib.pack_seqs(seqs)
        cols = np.sort(rng.choice(n, size=n // 2, replace=False))
        t0 = time.time()
        insert = st.res.fn("insert_kmers")
        for c in cols:
            check(insert(st.res.ix, int(c), blob, _lib.ptr(off), len(seqs), k))
        check(L.bigsi_hip_synchronize(st.handle))
        plant_s = time.time() - t0
    blob, off = _lib.pack_seqs(seqs)
    n_groups = 2 if call.endswith("2") else 64
    group_of = (np.arange(n, dtype=np.uint64) % n_groups).astype(np.uint32)
    if call == "tally":
        t = st.new_tally()

        def one():
            t.reset()
            check(L.bigsi_hip_tally_add_stream(t.b, blob, _lib.ptr(off), len(seqs), k, 1.0))
            return int(t.fetch()[0].sum())
    elif call.startswith("classify"):
        records = np.zeros(len(seqs), RECORD_DTYPE)

        def one():
            check(L.bigsi_hip_classify_stream(st.handle, blob, _lib.ptr(off), len(seqs), k, 1.0, _lib.ptr(group_of), n, n_groups, _lib.ptr(records)))
            return int(records["samples_hit"].astype(np.uint64).sum())
    else:
        counts, info = np.zeros((len(seqs), n_groups), np.uint32), np.zeros(len(seqs), INFO_DTYPE)

        def one():
            check(L.bigsi_hip_associate_stream(st.handle, blob, _lib.ptr(off), len(seqs), k, 1.0, _lib.ptr(group_of), n, n_groups, _lib.ptr(counts), _lib.ptr(info)))
            assert int(counts.astype(np.uint64).sum()) == int(info["grouped_hit"].astype(np.uint64).sum()) == int(info["samples_hit"].astype(np.uint64).sum())
            return int(info["samples_hit"].astype(np.uint64).sum())
    one()
    walls = []
    for _ in range(3):
        t0 = time.perf_counter()
        hits = one()
        walls.append((time.perf_counter() - t0) * 1e3)
    check(L.bigsi_hip_set_profiling(st.handle, 1))
    stats(st)
    one()
    s_ = stats(st)
    check(L.bigsi_hip_set_profiling(st.handle, 0))
    emit("associate_" + inp, call=call, threshold=1.0, n_seqs=len(seqs), cols=n, n_groups=None if call == "tally" else n_groups, hit_columns=hits,
         call_ms=min(walls), call_ms_all=walls, consumer_kernels_ms=s_.compact_ms, row_and_ms=s_.and_ms, k1_ms=s_.kmerize_ms,
         note="fill %.1f s, planted in %.1f s; a process of its own" % (fill_s, plant_s))
    if call == "tally":
        t.close()
    st.delete_all()


def window():
    """Windowed search (bigsi_hip_window_search): one 100 kbp query, W = 1000, t = 0.9 on the C3 index (10 M x 100 k, h = 4); a 1.5 kbp
    stretch of the query is planted in eight samples so that the call has hits to locate.  Per call: the wall clock, the window kernels by
    the library's HIP events on the index stream (k_window_max + k_window_combine + K4 + k_window_bits + k_window_locate: presence_ms of
    bigsi_hip_stats; the split per kernel is this command under `rocprofv3 --kernel-trace --stats`) and the exact run in front of them.
    Algorithmic bytes of the sweep: 2 h rows per window start plus We h rows of warm-up per segment, times the row bytes.  Beside it, in
    the same session and alternating with it: the row-AND kernel's rate on the same query (an exact batch run) and the only route to the
    same answer without the feature -- the windows as separate queries through bigsi_hip_search_stream at the same threshold (the
    counting path), every BIGSI_WINDOW_EVERY-th start (default 64) timed and scaled to all of them, labelled as a scaling.
    BIGSI_WINDOW_SHAPE="MxNxHxQLENxW" replaces the shape."""
    L, C = _lib.lib(), _lib.C
    m, n, h, qlen, w = 10_000_000, 100_000, 4, 100_000, 1000
    if os.environ.get("BIGSI_WINDOW_SHAPE"):
        m, n, h, qlen, w = (int(x) for x in os.environ["BIGSI_WINDOW_SHAPE"].split("x"))
    every, t, k = int(os.environ.get("BIGSI_WINDOW_EVERY", "64")), 0.9, 31
    st, fill = open_index("window", m, n, h)
    wv = -(-n // 64)
    rng = np.random.default_rng(23)
    query = rand_seqs(rng, 1, qlen)[0]
    for c in range(8):
        st.insert_kmers(1000 + 12_000 * c, [query[qlen // 5:qlen // 5 + 1500]], k)
    npos = qlen - k + 1
    starts = npos - w + 1
    tiles = -(-wv // 128)
    seg = min(max(-(-starts // max(-(-4096 // tiles), 1)), max(w, 64)), max(4 * w, 64))          # plan_window_search
    n_segs = -(-starts // seg)
    ab = (2 * h * (starts - n_segs) + w * h * n_segs) * wv * 8
    unique = len({query[i:i + k] for i in range(npos)})
    ab_and = unique * h * wv * 8
    batch = st.new_batch([query], k)
    subs = [query[s:s + w + k - 1] for s in range(0, starts, every)]
    st.window_search([query], k, w, t)                  # warm: the workspace's allocations
    batch.run(1.0)
    st.search_many(subs[:8], k, t)
    for rep in range(3):                                # the three legs alternate in one session
        check(L.bigsi_hip_set_profiling(st.handle, 1))
        stats(st)
        t0 = time.perf_counter()
        used, need, off, cols, recs = st.window_search([query], k, w, t)
        call = (time.perf_counter() - t0) * 1e3
        s_ = stats(st)
        batch.run(1.0)
        check(L.bigsi_hip_synchronize(st.handle))
        sa = stats(st)
        check(L.bigsi_hip_set_profiling(st.handle, 0))
        t0 = time.perf_counter()
        _, _, hoff, hcol, _ = st.search_many(subs, k, t)
        sub_ms = (time.perf_counter() - t0) * 1e3
        win_ms = s_.presence_ms
        emit("window_search", rep=rep, m=m, cols=n, h=h, query_bp=qlen, window=w, threshold=t, positions=npos, starts=starts, segment_starts=seg,
             segments=n_segs, hits=int(off[-1]), best_found_max=int(recs["best_found"].max()) if len(recs) else 0, call_ms=call,
             window_kernels_ms=win_ms, exact_run_ms=s_.and_ms + s_.kmerize_ms + s_.compact_ms, alg_bytes=ab,
             window_kernels_GBps=ab / win_ms / 1e6 if win_ms else None, row_and_ms=sa.and_ms, row_and_alg_bytes=ab_and,
             row_and_GBps=ab_and / sa.and_ms / 1e6 if sa.and_ms else None, windows_as_queries=len(subs), windows_as_queries_ms=sub_ms,
             windows_as_queries_hits=int(hoff[-1]), all_windows_scaled_ms=sub_ms * starts / len(subs), scaled_over_call=sub_ms * starts / len(subs) / call,
             note="fill %.2f s; every %d-th window start timed through search_stream and SCALED to all %d starts" % (fill, every, starts))
    batch.close()
    st.delete_all()


def genotype():
    """Panel genotyping (BIGSI.genotype_panel, bigsi_hip_genotype) beside the route without the feature, BIGSIVariantSearch.genotype_many
    (one search_batch at threshold 1, a list of sample-name dicts per probe, Python sets), on one hit-dense index: N samples, V variants
    with one 41-base ref and one alt probe each, every ref probe held by every sample and the alt probe of every 10th variant by every
    other sample.  Wall clock, best of 3 calls each, one process; the two results are compared call for call.
    BIGSI_GENOTYPE_SHAPE="NxV" replaces the shape."""
    import bigsi_amd
    from bigsi_amd.genotype import parse_panel
    from bigsi_amd.utils import seq_to_kmers
    from bigsi_amd.variant_search import BIGSIVariantSearch
    n, v_n, k, m, h = 20_000, 200, 21, 20011, 3
    if os.environ.get("BIGSI_GENOTYPE_SHAPE"):
        n, v_n = (int(x) for x in os.environ["BIGSI_GENOTYPE_SHAPE"].split("x"))
    rng = np.random.default_rng(5)
    refs = rand_seqs(rng, v_n, 41)
    alts = [r[:20] + ("A" if r[20] != "A" else "C") + r[21:] for r in refs]
    cfg = {"storage-engine": "hip-hbm", "storage-config": {"name": "measure_genotype"}, "k": k, "m": m, "h": h}
    kr = [km for r in refs for km in seq_to_kmers(r, k)]
    ka = [km for v, a in enumerate(alts) if v % 10 == 0 for km in seq_to_kmers(a, k)]
    every, other = bigsi_amd.BIGSI.bloom(cfg, kr), bigsi_amd.BIGSI.bloom(cfg, kr + ka)
    b = bigsi_amd.BIGSI.build(cfg, [other if s % 2 else every for s in range(n)], ["s%d" % s for s in range(n)])
    panel = "".join(">ref-V%d?x\n%s\n>alt-V%d-0\n%s\n" % (v, r, v, a) for v, (r, a) in enumerate(zip(refs, alts)))
    _, probes, allele_of = parse_panel(panel)
    vs = BIGSIVariantSearch(b, "ref.fa")

    def best(fn):
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            out = fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return min(ms), out
    try:
        many_ms, many = best(lambda: vs.genotype_many([([r], [a]) for r, a in zip(refs, alts)]))
        panel_ms, res = best(lambda: b.genotype_panel(panel))
        summary_ms, _ = best(lambda: b.genotype_panel(panel, summary_only=True))
        arrays_ms, _ = best(lambda: b.genotype_arrays(probes, allele_of, v_n))
        for var, one in zip(res["variants"], many):
            assert var["calls"] == {r["sample_name"]: r["genotype"] for r in one}
        emit("genotype", samples=n, variants=v_n, probes=len(probes), calls=sum(len(one) for one in many), het=sum(var["counts"]["0/1"] for var in res["variants"]),
             genotype_many_ms=many_ms, genotype_panel_ms=panel_ms, genotype_panel_summary_ms=summary_ms, genotype_arrays_ms=arrays_ms,
             many_over_panel=many_ms / panel_ms, note="wall clock, best of 3; genotype_panel names every call, summary_only and genotype_arrays do not")
    finally:
        b.delete()


def typing():
    """Locus typing (BIGSI.type_samples, bigsi_hip_typing) beside the route without the feature -- search_stream of the scheme's records
    at the same threshold, then the argmax over every (record, sample) hit on the host -- on one hit-dense index: N samples, a scheme
    of L loci and A alleles in all (120 bases each, the alleles of a locus two substitutions away from the locus's base sequence),
    every sample holding one allele of every locus.  Below threshold 1 several alleles of a locus hit every sample and the fraction
    decides.  Wall clock, best of 3 calls each, one process; the two routes' calls are compared cell for cell.
    BIGSI_TYPING_SHAPE="NxLxA" replaces the shape, BIGSI_TYPING_THRESHOLD the threshold."""
    import bigsi_amd
    from bigsi_amd.locus_typing import EXACT_SCORE, parse_scheme
    from bigsi_amd.utils import seq_to_kmers
    n, n_loci, n_alleles, k, m, h = 20_000, 7, 200, 21, 200003, 3
    if os.environ.get("BIGSI_TYPING_SHAPE"):
        n, n_loci, n_alleles = (int(x) for x in os.environ["BIGSI_TYPING_SHAPE"].split("x"))
    thr = float(os.environ.get("BIGSI_TYPING_THRESHOLD", "0.5"))
    rng = np.random.default_rng(7)
    per = [n_alleles // n_loci + (1 if l < n_alleles % n_loci else 0) for l in range(n_loci)]
    alleles = []
    for l, base in enumerate(rand_seqs(rng, n_loci, 120)):
        one = []
        for a in range(per[l]):
            s = list(base)
            for pos in rng.choice(120, size=2, replace=False):
                s[pos] = "ACGT"[("ACGT".index(s[pos]) + 1 + int(rng.integers(3))) % 4]
            one.append("".join(s))
        alleles.append(one)
    scheme = "".join(">locus%d_%d\n%s\n" % (l, a + 1, s) for l, one in enumerate(alleles) for a, s in enumerate(one))
    cfg = {"storage-engine": "hip-hbm", "storage-config": {"name": "measure_typing"}, "k": k, "m": m, "h": h}
    blooms = {}
    for s in range(n):
        combo = tuple(s % c for c in per)
        if combo not in blooms:
            blooms[combo] = bigsi_amd.BIGSI.bloom(cfg, [km for l, a in enumerate(combo) for km in seq_to_kmers(alleles[l][a], k)])
    b = bigsi_amd.BIGSI.build(cfg, [blooms[tuple(s % c for c in per)] for s in range(n)], ["s%d" % s for s in range(n)])
    loci, names, labels, records, locus_of, allele_of = parse_scheme(scheme)

    def best(fn):
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            out = fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return min(ms), out

    def host_route():
        """the parent's route: every hit as a result dict, the argmax in Python"""
        top, dicts = {}, 0
        for pos, (_, results) in enumerate(b.search_stream(records, thr)):
            l, ident = int(locus_of[pos]), int(allele_of[pos])
            for r in results:
                dicts += 1
                key = (r["num_kmers_found"] * EXACT_SCORE // r["num_kmers"], -ident)
                cell = (l, r["sample_name"])
                if key > top.get(cell, (-1, 0)):
                    top[cell] = key
        return top, dicts
    try:
        host_ms, (top, dicts) = best(host_route)
        typed_ms, res = best(lambda: b.type_samples(scheme, threshold=thr))
        summary_ms, summary = best(lambda: b.type_samples(scheme, threshold=thr, summary_only=True))
        arrays_ms, arrays = best(lambda: b.typing_arrays(records, locus_of, len(loci), thr, allele_of=allele_of))
        cells = 0
        for s in res["samples"]:
            for l, name in enumerate(loci):
                c, want = s["calls"].get(name), top.get((l, s["sample_name"]))
                assert (c is None) == (want is None), (s["sample_name"], name)
                if c is not None:
                    assert c["allele"] == labels[-want[1]] and c["fraction"] == want[0] / float(EXACT_SCORE), (s["sample_name"], name, c, want)
                    cells += 1
        assert cells == len(top) == sum(x["called"] for x in res["loci"]) and summary["loci"] == res["loci"]
        emit("typing", samples=n, loci=len(loci), alleles=len(records), threshold=thr, called_cells=cells, exact_cells=sum(x["exact"] for x in res["loci"]),
             multiple_cells=sum(x["multiple"] for x in res["loci"]), result_dicts=dicts, search_stream_argmax_ms=host_ms, type_samples_ms=typed_ms,
             type_samples_summary_ms=summary_ms, typing_arrays_ms=arrays_ms, host_over_typed=host_ms / typed_ms, host_over_arrays=host_ms / arrays_ms,
             cell_bytes_out=int(arrays[0].nbytes + arrays[1].nbytes), count_bytes_out=int(arrays[2].nbytes + arrays[3].nbytes + arrays[4].nbytes),
             note="wall clock, best of 3; type_samples names every call, summary_only downloads the counts only, typing_arrays the cells as arrays")
    finally:
        b.delete()


if __name__ == "__main__":
    todo = sys.argv[1:] or ["c2stream", "c3batch", "p16", "c4shard", "northstar", "k5", "transpose"]
    for t in todo:
        globals()[t]()
