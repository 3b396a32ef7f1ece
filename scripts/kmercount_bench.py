#!/usr/bin/env python
"""Ingest rate of the exact k-mer counter: KmerCounter.add + bloom on synthetic reads (150-base reads at 30x over a 5 Mb random genome
with 1 % substitutions unless told otherwise), beside three yardsticks for the same bytes -- a single-threaded host copy (what the
staging of a chunk costs the host: its share of the add time is reported), the bare pinned host-to-device copy (the bound the staging
cannot beat) and the host twin (libbigsi_cpu.so, one core, on a fraction of the reads).  Prints one JSON line.  Not part of bench.py:
the headline benchmark measures search."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_reads(genome_bases, coverage, read_length, error, seed):
    """(uint8 blob of ACGT bytes, uint64 offsets): reads from both strands of a random genome, each base substituted with probability `error`."""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, genome_bases, dtype=np.uint8)
    n = int(genome_bases * coverage / read_length)
    starts = rng.integers(0, genome_bases - read_length + 1, n)
    codes = genome[starts[:, None] + np.arange(read_length)[None, :]]
    flip = rng.random(n) < 0.5
    codes[flip] = 3 - codes[flip, ::-1]
    wrong = rng.random(codes.shape) < error
    codes[wrong] = (codes[wrong] + rng.integers(1, 4, int(wrong.sum()), dtype=np.uint8)) & 3
    blob = np.frombuffer(b"ACGT", np.uint8)[codes].reshape(-1)
    return np.ascontiguousarray(blob), np.arange(n + 1, dtype=np.uint64) * np.uint64(read_length)


def best(fn, reps):
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t)
    return min(times), times


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--coverage", type=float, default=30.0)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("-k", type=int, default=31)
    ap.add_argument("-m", type=int, default=25_000_000)
    ap.add_argument("--hashes", type=int, default=3)
    ap.add_argument("--min-count", type=int, default=2)
    ap.add_argument("--expected-distinct", type=int, default=0, help="sizing hint handed to the counter (0: let the table grow)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--twin-fraction", type=float, default=0.02, help="share of the reads the host twin counts (a std::map on one core)")
    ap.add_argument("--reads", choices=["synthetic", "homopolymer"], default="synthetic",
                    help="homopolymer: the same number of reads of the same length, all C -- every wavefront's windows combine into one table atomic, so "
                         "k_count_kmers' time under a kernel trace is its cost without the table (LDS codes, rolling, combining)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args(argv)

    import torch
    from bigsi_amd.kmercount import KmerCounter
    blob, off = synthetic_reads(a.genome, a.coverage, a.read_length, a.error, a.seed)
    if a.reads == "homopolymer":
        blob = np.full_like(blob, ord("C"))
    bases = int(blob.size)
    out = {"reads_kind": a.reads, "bases": bases, "reads": int(off.size - 1), "k": a.k, "m": a.m, "h": a.hashes, "min_count": a.min_count, "reps": a.reps}

    info = {}

    def ingest():
        with KmerCounter(a.k, expected_distinct=a.expected_distinct, device=a.device) as c:
            t0 = time.perf_counter()
            c.add_packed(blob, off)
            t1 = time.perf_counter()
            c.bloom_bytes(a.m, a.hashes, a.min_count)
            t2 = time.perf_counter()
            info.update(c.info(), add_seconds=t1 - t0, bloom_seconds=t2 - t1, kept=int(c.spectrum()[a.min_count:].sum()))

    ingest()          # warm-up: module load, pinned and device allocations of the runtime
    total, all_times = best(ingest, a.reps)
    out.update(info, seconds=total, all_seconds=all_times, bases_per_second=bases / total)

    dst = np.empty_like(blob)
    copy_s, _ = best(lambda: np.copyto(dst, blob), a.reps)
    out.update(host_copy_seconds=copy_s, host_copy_share_of_add=copy_s / info["add_seconds"])

    pinned = torch.from_numpy(blob).pin_memory()
    dev = torch.empty(bases, dtype=torch.uint8, device="cuda:%d" % a.device)

    def h2d():
        dev.copy_(pinned, non_blocking=True)
        torch.cuda.synchronize(a.device)

    h2d()
    h2d_s, _ = best(h2d, a.reps)
    out.update(h2d_seconds=h2d_s, h2d_gbytes_per_second=bases / h2d_s / 1e9)

    n_twin = max(int((off.size - 1) * a.twin_fraction), 1)
    twin_bases = int(off[n_twin])
    with KmerCounter(a.k, library="cpu") as c:
        t = time.perf_counter()
        c.add_packed(blob[:twin_bases], off[:n_twin + 1])
        c.bloom_bytes(a.m, a.hashes, a.min_count)
        twin_s = time.perf_counter() - t
    out.update(twin_bases=twin_bases, twin_seconds=twin_s, twin_bases_per_second=twin_bases / twin_s)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
