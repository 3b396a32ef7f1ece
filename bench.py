#!/usr/bin/env python
"""bench.py -- BIGSI query hot path on MI355X: k-mer lookups/s and achieved HBM GB/s of the row-fetch-AND kernel.

    python bench.py --gpus N --steps K --warmup W [--workload c3|c2|c4|c5|northstar] [--threshold T]

With N > 1 and no launcher environment the script starts its own N ranks (one process per GPU, RANK / LOCAL_RANK /
WORLD_SIZE / MASTER_* set for them); under `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N` it is
one of the launcher's ranks.  Either way rank 0 prints ONE JSON line.

A "step" is one pass of the whole path over one batch of synthetic queries, HOST-VISIBLE as SURVEY.md section 8d defines
lookups/s (--timed host, the default): the batch's sequences start in host memory, its hit lists end in host memory -- on one
GPU one bigsi_hip_search_stream call per step (the library cuts the batch into device chunks and overlaps upload, kernels and
download itself), with N > 1 the batch object's reload + sharded run + fetch of the gathered lists.  The index is resident in
HBM throughout.  (--timed resident, and always for score=True workloads and for batches of short reads -- c2's 1000 x 61 bp are one 48 us call,
latency not throughput; their host-visible rate is that of one stream call over 256 batches, `hv` --: the batch is staged in HBM beforehand and the hit
lists stay on the device -- that figure is also measured after a host-timed region: config.resident_lookups_per_s.)  The path:
K1 k-merise/dedupe/hash -> K2 row fetch + AND (or bit-sliced counting) -> K4 threshold + compaction, and for N > 1 the RCCL
all-gather of the per-sample result vectors, the compaction of the gathered result and (thresholded searches) the all-reduce
of the per-hit counts, issued by libbigsi_hip.so on its own communicator.

Workloads are BASELINE.json's configurations; each names a WHOLE index, which is split by column range over the N GPUs
(strong scaling: total work fixed).  `value` = unique query k-mers looked up in the WHOLE index per second of wall time,
exchange included -- every rank looks every k-mer up in its shard, so the shard-level lookups/s summed over ranks
(config.shard_lookups_per_s_sum) is N times that and is NOT the headline.
    c3 (default)  BASELINE configs[2]: 10M rows x 100k samples (125 GB), h=4, 8192 x 1 kbp queries, threshold 1.0
    c2            BASELINE configs[1]: 1M x 10k, h=3, 1000 x 61-mers, a different batch every step (32 staged batches cycle)
    c4            BASELINE configs[3]: 25M x 500k, h=3 (1.56 TB: needs 8 GPUs), 256 x 1 kbp queries per step
    c5            BASELINE configs[4]: c4 at threshold 0.4 with score=True: every step also brings the hit lists to the host and
                  runs the whole scored path for them -- K5 + K6 on the device (presence bits, run tallies, the rounded score chain),
                  closed-form score fields, presence strings and result dicts on the host -- one batch behind the launches;
                  16 queries x 16 planted samples per shard and batch
    northstar     BASELINE north_star: 10M x 500k, h=3 (625 GB: needs >= 4 GPUs)
`--shard-of P` runs, on fewer GPUs, the first N of the P column shards of the workload (e.g. `--workload c4 --shard-of 8
--gpus 1` is what one GPU of the 8-GPU C4 run does; value is then the rate against that part of the index and says so).
`--scaling weak` instead gives every GPU the workload's whole shape (index = N x the columns).

THE LINE.  Rank 0 prints one JSON line of at most 7.5 KB (the driver keeps 8 KB of stdout): flat, short keys, prose cut to
< 120 characters; `--details FILE` also writes the verbose record (everything this script measured, with units and
explanations) -- profiles/ holds those of the builder's own runs.

A plain run sets up, warms up, times the --steps steps and prints the line (`value`, `ms_per_step` and the workload's shape);
`--dump-outputs DIR` also writes what the last timed step computed -- always the first staged batch, the one with the planted hits
(up to distinct-batches - 1 untimed warmup steps are added for that).  `--full` adds everything else this script measures or checks:
the verification against the oracle, roofline and same-box calibration, the resident / host-visible / one-call figures, clocks,
the CPU baseline and, for the default command, the other BASELINE configurations as legs of >= 1 s each, every one a fresh process
verified against the oracle, under config.also (N > 1: the legs run before the headline, while no rank holds its GPU):
    --gpus 1   c3 at 0.4, c2, c2 at 0.4, one GPU's shard (1 of 8) of c4 / c5 (scored) / north-star
    --gpus 2   c3 at 0.4 (the thresholded exchange: mask all-gather + count all-reduce)
    --gpus 4   north-star 10M x 500k as a WHOLE index over the 4 GPUs, c3 at 0.4
    --gpus 8   c4 25M x 500k, c5 (0.4, score=True in the step), north-star: WHOLE indexes over the 8 GPUs, c3 at 0.4
(legs of a multi-GPU run: every rank starts its rank of the leg, rendezvous on ports rank 0 drew before the headline's group
was closed).  Short keys of a leg: v lookups/s | ms per step | s timed | k kernel | f frac of 8 TB/s by the kernel's clock | sf
by the step's wall clock | box frac of this box's bare row-stream rate (bigsi_hip_probe_rows) | tr PMC traffic / algorithmic
bytes (tr5: K5's over the hit words' bytes, tr5l: over the bytes of the 128-byte lines they lie in -- the L2 never fetches less) | ok verified | in h: the leg's steps take host sequences in and leave host hit lists out (v is the host-visible rate, rv the rate with
the batches resident in HBM), r: resident steps (hv then = host-visible lookups/s of one search_stream call) | us1 one-call latency of one query | x_ms exchange
(all-gather + gathered compaction + all-reduce, events on the communicator stream) | ranks = ncclCommCount | gbs per-rank GB/s.
"""
import argparse
import json
import os

# multi-process GPU work on these hosts needs dmabuf IPC (RCCL across ranks fails with hipIpcGetMemHandle otherwise); the driver's
# environment exports it -- keep it if it does not.  Must be in place before any HIP runtime loads (torch, libbigsi_hip.so below)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
import shutil
import socket
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md: 8.0 TB/s; 6.29 TB/s measured copy)
HBM_BYTES = 288e9            # per GPU (spec); an index shard may take at most FIT_FRACTION of it
FIT_FRACTION = 0.93
SEED = 20260928

WORKLOADS = {
    "c2": dict(rows=1_000_000, cols=10_000, hashes=3, batch=1000, qlen=61, threshold=1.0, distinct=32, score=False,
               name="BASELINE configs[1]"),
    "c3": dict(rows=10_000_000, cols=100_000, hashes=4, batch=8192, qlen=1000, threshold=1.0, distinct=2, score=False,
               name="BASELINE configs[2]"),
    "c4": dict(rows=25_000_000, cols=500_000, hashes=3, batch=256, qlen=1000, threshold=1.0, distinct=2, score=False,
               name="BASELINE configs[3]"),
    "c5": dict(rows=25_000_000, cols=500_000, hashes=3, batch=256, qlen=1000, threshold=0.4, distinct=2, score=True,
               name="BASELINE configs[4]"),
    "northstar": dict(rows=10_000_000, cols=500_000, hashes=3, batch=256, qlen=1000, threshold=1.0, distinct=2, score=False,
                      name="BASELINE north_star shape"),
}


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--workload", default="c3", choices=sorted(WORKLOADS))
    p.add_argument("--scaling", default="strong", choices=["strong", "weak"])
    p.add_argument("--shard-of", type=int, default=0, help="hold the first --gpus of this many column shards of the workload")
    # overrides of the workload's shape (ad-hoc runs, tests)
    p.add_argument("--rows", type=int)
    p.add_argument("--cols", type=int, help="sample columns of the WHOLE index (strong) / per GPU (weak)")
    p.add_argument("--hashes", type=int)
    p.add_argument("--batch", type=int)
    p.add_argument("--qlen", type=int)
    p.add_argument("--threshold", type=float)
    p.add_argument("--distinct-batches", type=int, help="staged query batches the steps cycle through")
    p.add_argument("--score", type=int, choices=[0, 1])
    p.add_argument("--k", type=int, default=31)
    p.add_argument("--and-draws", type=int, default=2, help="bit density of the synthetic index = 2^-draws")
    p.add_argument("--full", action="store_true",
                   help="measure and check everything beside the headline (see the module docstring); a plain run sets up, warms up, times "
                        "the steps and prints the line")
    p.add_argument("--dump-outputs", metavar="DIR",
                   help="after the timed steps, write what the last of them computed (the arrays its caller receives) as DIR/<name>.npy "
                        "in float64, at most 64 MB in all")
    p.add_argument("--cpu-seconds", type=float, default=12.0, help="--full: budget of the CPU baseline sample (0 = skip)")
    p.add_argument("--cpu-rows", type=int, default=200_000)
    p.add_argument("--dense", type=int, default=0, choices=[0, 1],
                   help="the hit-dense variant of the workload (what real thresholded searches produce; the plain workloads carry ~1 hit per query): "
                        "gene-length queries: the first 16 queries of every batch are held, up to 15 SNPs apart, by 1 %% of the shard's samples "
                        "(~625 hits per query at 62.5 k samples, ~10 k per batch); reads: every read is held by 8 samples")
    p.add_argument("--early-exit", type=int, default=0, choices=[0, 1],
                   help="run with the library's opt-in early exit (a wavefront stops fetching a query's rows for its column segment once no sample "
                        "there can still reach the threshold): same hit lists, FEWER bytes than the reference reads -- reported as legs beside "
                        "the plain figures, never as the headline; roofline figures of such a run price the ALGORITHMIC bytes, not the bytes read")
    p.add_argument("--no-verify", action="store_true")
    p.add_argument("--score-queue", default="beside", choices=["ordered", "beside"],
                   help="score=True workloads: K5 + K6 of a batch queued on the index stream behind the next batch's kernels (ordered) or on "
                        "the library's high-priority score stream beside them (beside)")
    p.add_argument("--timed", default="host", choices=["host", "resident"],
                   help="what a timed step starts from and leaves behind.  host (default; SURVEY.md section 8d metric (1)): the step's sequences are in HOST memory "
                        "and its hit lists end in host memory -- one bigsi_hip_search_stream call per step on one GPU (the library uploads, runs and downloads its "
                        "own chunks, overlapped); N > 1: reload (H2D) + sharded run + fetch of the previous batch's gathered hit lists.  resident: the "
                        "round 1-5 step (batches staged in HBM beforehand, hit lists left on the device); it is also measured after a host-timed region "
                        "and reported as config.resident_lookups_per_s.  score=True workloads, batches of short reads (< 128 KB of sequence: one latency-bound call) "
                        "and --one-stream always run resident steps")
    p.add_argument("--host-visible", type=int, default=1, choices=[0, 1],
                   help="0: skip the host-visible measurements after the timed region (profiled runs: rocprofv3's per-kernel averages then "
                        "cover launches of the timed shape only)")
    p.add_argument("--also", default="auto", choices=["auto", "all", "none"],
                   help="--full: run short legs of the other BASELINE configurations and report them under config.also "
                        "(auto: only for the default c3 command)")
    p.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo for several ranks on one GPU)")
    p.add_argument("--one-device", action="store_true", help="every rank uses device 0 (dry runs of the N>1 path on a 1-GPU box; needs --backend gloo)")
    p.add_argument("--one-stream", action="store_true", help="read workloads: every step on the index stream (no overlap of consecutive launches): the A/B "
                                                            "switch behind roofline.kernel_ms of such workloads")
    p.add_argument("--alone-steps", type=int, default=400, help="read workloads: steps of the untimed one-stream pass that prices the kernel alone on the device (0 = skip)")
    p.add_argument("--details", help="also write the verbose record (JSON) to this file")
    p.add_argument("--rows-cap", type=int, default=0, help="cut every workload's rows to at most this many (dry runs of the multi-GPU command on one GPU)")
    p.add_argument("--leg-seconds", type=float, default=1.0, help="timed seconds each config.also leg aims at")
    p.add_argument("--force-dist", action="store_true",
                   help="initialise the process group and take the exchange path even with one rank (exercises the N>1 code)")
    a = p.parse_args()
    if a.steps < 1 or a.warmup < 0:
        p.error("--steps must be at least 1 and --warmup at least 0")
    w = dict(WORKLOADS[a.workload])
    a.custom = []
    for key, arg in (("rows", a.rows), ("cols", a.cols), ("hashes", a.hashes), ("batch", a.batch), ("qlen", a.qlen),
                     ("threshold", a.threshold), ("distinct", a.distinct_batches), ("score", a.score)):
        if arg is not None:
            w[key] = type(w[key])(arg)
            a.custom.append(key)
    if a.rows_cap and w["rows"] > a.rows_cap:
        w["rows"] = a.rows_cap
        a.custom.append("rows<=%d" % a.rows_cap)
    a.w = w
    return a


def rand_seqs(rng, n, qlen):
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    return [lut[r].tobytes().decode("ascii") for r in rng.integers(0, 4, size=(n, qlen), dtype=np.uint8)]


# ------------------------------------------------------------------------------------------------ hit-dense variants (--dense 1)
DENSE_QUERIES, DENSE_COL_FRACTION, DENSE_MAX_SNPS, DENSE_READ_HITS = 16, 0.01, 15, 8


def dense_gene_plants(w, nb, g, cols_g, k):
    """Gene-length workloads: the first DENSE_QUERIES queries of every staged batch are shared -- 0 to DENSE_MAX_SNPS SNPs apart, so
    that the presence strings carry the gaps the scorer is about -- by DENSE_COL_FRACTION of the shard's samples.  Yields
    (batch, query, cols int64[], segs) with segs[j] = [(a, b), ...]: the stretches of the query that sample cols[j] holds."""
    for bi in range(nb):
        for qi in range(min(DENSE_QUERIES, w["batch"])):
            rng = np.random.default_rng([SEED, 77, g, bi, qi])
            cols = np.sort(rng.choice(cols_g, size=max(1, int(cols_g * DENSE_COL_FRACTION)), replace=False))
            segs = []
            for _ in cols:
                n_snps = int(rng.integers(0, DENSE_MAX_SNPS + 1))
                cuts = [-1] + np.sort(rng.choice(w["qlen"], size=n_snps, replace=False)).tolist() + [w["qlen"]]
                segs.append([(a + 1, b) for a, b in zip(cuts[:-1], cuts[1:]) if b - a - 1 >= k])
            yield bi, qi, cols, segs


def seg_masks(segs, n_kmers, k):
    """bool[len(segs), n_kmers]: k-mer position i lies inside one of sample j's stretches"""
    out = np.zeros((len(segs), n_kmers), dtype=bool)
    for j, sg in enumerate(segs):
        for a, b in sg:
            out[j, a:b - k + 1] = True
    return out


def dense_read_cols(bi, r, g, cols_g):
    """Read workloads: the DENSE_READ_HITS samples that hold read r of staged batch bi (whole)."""
    return [(7919 * (DENSE_READ_HITS * r + t) + 101 * bi + 13 * g) % cols_g for t in range(DENSE_READ_HITS)]


# ------------------------------------------------------------------------------------------------ self launch
def self_launch(args):
    """--gpus N without a launcher: start N ranks of this script, wait, relay rank 0's JSON line."""
    n = args.gpus
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out0 = tempfile.NamedTemporaryFile("w+", prefix="bigsi_bench_rank0_", suffix=".out", delete=False)
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      stdout=out0 if r == 0 else sys.stderr, stderr=sys.stderr))
    rc = 0
    try:
        while any(p.poll() is None for p in procs):
            bad = [p for p in procs if p.poll() not in (None, 0)]
            if bad:                    # one rank died: the others would wait for it in a collective for ever
                rc = bad[0].returncode
                break
            time.sleep(0.2)
    finally:
        for p in procs:
            if p.poll() is None:
                p.terminate() if rc else p.wait()
        for p in procs:
            try:
                p.wait(timeout=30)
            except subprocess.TimeoutExpired:
                p.kill()
    rc = rc or max(abs(p.returncode or 0) for p in procs)
    out0.seek(0)
    text = out0.read()
    out0.close()
    os.unlink(out0.name)
    if rc:
        sys.stderr.write(text)
        raise SystemExit("bench.py: a rank failed (exit code %d)" % rc)
    sys.stdout.write(text)
    sys.stdout.flush()


def cpu_baseline(args, w, cols_cpu, exact):
    """The CPU baseline beside the number (never the target), each leg in a fresh subprocess (fork pools must not inherit a HIP
    context), on the GPU run's synthetic index at full row width with the rows reduced to fit host RAM:
      * THROUGH THE PRODUCT BOUNDARY: libbigsi_cpu.so (include/bigsi_cpu.h, the CPU twin of the C ABI) -- reference-shaped on ONE core
        (the reported `value`), the reference's process-pool-over-sequences parallelism (bulk_search) on every physical core, and
        its word-parallel mode on one core ("best CPU");
      * the oracle's C port (oracle/bigsi_oracle.c, test infrastructure), one core and pool, as a cross-check of the twin."""
    rows, batch = min(w["rows"], args.cpu_rows), min(w["batch"], 256)
    common = ["--rows", str(rows), "--cols", str(cols_cpu), "--hashes", str(w["hashes"]), "--k", str(args.k), "--and-draws", str(args.and_draws),
              "--seed", str(SEED), "--batch", str(batch), "--qlen", str(w["qlen"]), "--exact", str(int(exact))]
    sec = max(args.cpu_seconds / 4.0, 1.0)
    t = json.loads(subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "cpu_twin_baseline.py")] + common +
                                  ["--threshold", str(w["threshold"]), "--seconds", str(sec), "--pool-runs", "2"],
                                  check=True, capture_output=True, text=True, timeout=900).stdout.strip().splitlines()[-1])
    r = json.loads(subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "cpu_baseline.py")] + common +
                                  ["--seconds", str(sec), "--pool-runs", "2", "--pool-seconds", str(max(args.cpu_seconds / 6.0, 1.0))],
                                  check=True, capture_output=True, text=True, timeout=900).stdout.strip().splitlines()[-1])
    what = "%d-row x %d-sample slice of the same synthetic index (full row width of one GPU's shard, rows reduced to fit host RAM), cycling over %d of the bench's queries; rows served from RAM instead of BerkeleyDB" % (rows, cols_cpu, batch)
    return {"sample_short": "%d lookups in %.1f s; %d-row x %d-sample slice of the same index in RAM (not BerkeleyDB), %d of the bench's queries"
                            % (t["one_core"]["lookups"], t["one_core"]["seconds"], rows, cols_cpu, batch),
            "value": t["one_core"]["rate"], "unit": "kmer_lookups/s", "cores": 1, "kind": "port",
            "through": "libbigsi_cpu.so: bigsi_cpu_search_batch, the CPU twin of the C ABI (include/bigsi_cpu.h), reference-shaped (per-k-mer string "
                       "canonicalisation, MurmurHash3 x h, one copy per fetched row, byte-wise AND, unpack-to-int32-and-add)",
            "sample": "%d unique k-mer lookups in %.1f s on a %s" % (t["one_core"]["lookups"], t["one_core"]["seconds"], what),
            "pool": {"value": t["pool"]["rate_median"], "best": t["pool"]["rate_best"], "runs": t["pool"]["rates"], "cores": t["pool"]["threads"],
                     "host_threads": t["host_threads"],
                     "sample": "fork pool over query sequences (the reference's bulk_search parallelism), %d workers, median of %d runs of %.1f s"
                               % (t["pool"]["threads"], len(t["pool"]["rates"]), t["pool"]["seconds"])},
            "word_parallel_one_core": {"value": t["word_parallel_one_core"]["rate"], "what": "BIGSI_CPU_WORD_PARALLEL: 64-bit words of the resident rows, no copies"},
            "word_parallel_pool": {"value": t["word_parallel_pool"]["rate"], "cores": t["word_parallel_pool"]["threads"],
                                   "what": "the same in the fork pool: the best this host's CPUs do on the path"},
            # the closest stand-in for north_star's "berkeleydb / CPU path" these hosts allow (no bsddb3, no libdb headers): the same
            # reference-shaped searches with every row read from a BerkeleyDB hash file that libdb itself wrote (tmpfs: page cache)
            "bdb_file": None if not t.get("bdb_file") else {"value": t["bdb_file"]["one_core"]["rate"], "pool": t["bdb_file"]["pool"]["rate"], "pool_cores": t["bdb_file"]["pool"]["threads"],
                                                            "file_gb": t["bdb_file"]["file_gb"], "what": t["bdb_file"]["what"]},
            "oracle_port": {"value": r["one_core"]["rate"], "pool": r["pool"]["rate_median"], "pool_cores": r["pool"]["threads"],
                            "what": "oracle/bigsi_oracle.c orc_query (test infrastructure), same slice and queries: cross-check of the twin"}}


ALSO_LEGS = {
    # world size -> [(key, what, arguments, steps for ~1 s of timed work)]: every leg is this script again in a fresh process (one per
    # rank), verified against the oracle in-run.  1 GPU: the other BASELINE configurations at the size one GPU holds; 4 / 8 GPUs: the
    # configurations that NEED that many GPUs, as whole indexes with the library's RCCL exchange.
    1: [("c3_t04", "configs[2] at threshold 0.4 (bit-sliced counting kernel)", ["--workload", "c3", "--threshold", "0.4"], 16),
        ("c2", "configs[1]: 1M x 10k, 1000 x 61-mers per step", ["--workload", "c2", "--warmup", "200"], 50000),
        ("c2_t04", "configs[1] at threshold 0.4", ["--workload", "c2", "--threshold", "0.4", "--warmup", "200"], 50000),
        ("c4_shard", "configs[3]: one GPU's shard (1 of 8) of 25M x 500k", ["--workload", "c4", "--shard-of", "8", "--warmup", "10"], 1200),
        ("c5_shard", "configs[4]: that shard at 0.4 with score=True in the step", ["--workload", "c5", "--shard-of", "8", "--warmup", "10"], 1000),
        ("ns_shard", "north_star 10M x 500k: one GPU's shard (1 of 8)", ["--workload", "northstar", "--shard-of", "8", "--warmup", "10"], 1200),
        # the hit-dense regime (every other leg carries ~1 hit per query: K4, the hit export, K5 / K6 and the host assembly idle there)
        ("c5_dense", "configs[4] shard, 16 of 256 queries held by 1 % of the samples (~10 k scored hits per batch)",
         ["--workload", "c5", "--shard-of", "8", "--dense", "1", "--warmup", "6"], 150),
        ("c2_dense", "configs[1], every read held by 8 samples", ["--workload", "c2", "--dense", "1", "--warmup", "200"], 30000),
        # opt-in early exit on the hit-dense index (NOT the reference's byte count: `tr` = bytes read / algorithmic bytes says how much less)
        ("c5_ee", "the c5_dense shard with early_exit (unscored step)", ["--workload", "c5", "--shard-of", "8", "--dense", "1", "--early-exit", "1", "--score", "0", "--warmup", "6"], 1500),
        # ... and on the headline's own workload: an exact search of the synthetic index settles every 8192-column segment after a dozen rows
        # (its ANDs run empty), so this leg reads a few per cent of the bytes -- what early_exit buys when queries do not match, not a lookup rate
        ("c3_ee", "configs[2] exact with early_exit (opt-in; reads a fraction of the algorithmic bytes)", ["--workload", "c3", "--early-exit", "1"], 350),
        # f1, index ingest: a 32 GB snapshot (device layout) written, dropped, loaded back (threads on the file, two pinned buffers,
        # asynchronous copies), sampled rows verified against the oracle's generator: scripts/ingest_bench.py, keys in GB/s
        ("ingest", "snapshot of a 32 GB index written / dropped / loaded back", ["--ingest", "32"], 0)],
    2: [("c3_t04", "configs[2] at threshold 0.4 over 2 GPUs", ["--workload", "c3", "--threshold", "0.4"], 32)],
    4: [("northstar", "north_star 10M x 500k, WHOLE index over 4 GPUs", ["--workload", "northstar", "--warmup", "10"], 700),
        ("c3_t04", "configs[2] at threshold 0.4 over 4 GPUs", ["--workload", "c3", "--threshold", "0.4"], 64)],
    8: [("c4", "configs[3]: 25M x 500k, WHOLE index over 8 GPUs, exact", ["--workload", "c4", "--warmup", "10"], 1200),
        ("c5", "configs[4]: the same at 0.4 with score=True in the step", ["--workload", "c5", "--warmup", "10"], 1000),
        ("northstar", "north_star 10M x 500k, WHOLE index over 8 GPUs", ["--workload", "northstar", "--warmup", "10"], 1200),
        ("c3_t04", "configs[2] at threshold 0.4 over 8 GPUs", ["--workload", "c3", "--threshold", "0.4"], 128)],
}
LEG_TIMEOUT_S = 300          # a leg that hangs (it never has) costs this much once: the legs after it are skipped


def also_legs_for(world):
    return ALSO_LEGS.get(world, [("c3_t04", "configs[2] at threshold 0.4 over %d GPUs" % world, ["--workload", "c3", "--threshold", "0.4"], 16 * world)])


def free_ports(n):
    socks, ports = [], []
    for _ in range(n):
        s_ = socket.socket()
        s_.bind(("127.0.0.1", 0))
        socks.append(s_)
        ports.append(s_.getsockname()[1])
    for s_ in socks:
        s_.close()
    return ports


def leg_summary(d, what, extra, wall_s):
    """A leg's own (condensed) line -> the few short keys the parent line carries for it (see the module docstring)."""
    rf, cf = d["roofline"], d["config"]
    out = {"v": d["value"], "ms": d["ms_per_step"], "s": sig(d["ms_per_step"] * d["steps"] / 1e3, 3), "k": rf.get("kernel"), "f": rf.get("frac"),
           "sf": rf.get("step_frac"), "box": rf.get("frac_of_box"), "tr": rf.get("traffic_ratio"), "ok": int(bool(cf.get("verified"))),
           "hv": cf.get("host_visible_lookups_per_s"), "rv": cf.get("resident_lookups_per_s"), "in": {"host": "h", "resident": "r"}.get(cf.get("value_inputs")), "us1": cf.get("one_call_us"), "gb": cf.get("index_gb_per_gpu"), "wall": wall_s}
    for k_src, k_dst in (("exchange_ms", "x_ms"), ("rccl_ranks", "ranks"), ("per_rank_GBps", "gbs"), ("scored_hits", "hits"), ("scored_us_per_hit", "us_hit"),
                         ("hv_scored_lookups_per_s", "hvs"), ("distinct_gpus", "gpus_distinct"), ("one_call_us_batch", "usb"), ("frac_overlapped", "f3"),
                         ("hits_per_s", "hps"), ("hv_hits_per_s", "hvh"), ("hv_scored_hits_per_s", "hvsh"), ("dicts_per_s", "dps"), ("k5_traffic_ratio", "tr5"), ("k5_line_ratio", "tr5l"),
                         ("k56_ms", "k56"), ("k56_GBps", "k56g"), ("early_exit", "ee")):
        v = cf.get(k_src, rf.get(k_src))
        if v is not None:
            out[k_dst] = v
    if cf.get("dense"):
        out["k4"] = rf.get("compact_ms")
    if rf.get("read_launches_repeated"):
        out["rep"] = rf["read_launches_repeated"]
    return {k_: v_ for k_, v_ in out.items() if v_ is not None}


def want_legs(args):
    return args.full and (args.also == "all" or (args.also == "auto" and args.workload == "c3" and not [c for c in args.custom if not c.startswith("rows<=")]
                                                 and not args.shard_of and args.scaling == "strong" and not args.force_dist and not args.one_stream))


def _sync_dir():
    # (keyed like _err_file; the legs rendezvous on 127.0.0.1, so all ranks of a run that has legs share this machine's temp dir)
    return os.path.join(tempfile.gettempdir(), "bigsi_bench_legs_%s_%d" % (os.environ.get("MASTER_PORT", "0"), os.getppid()))


def file_barrier(world, rank, tag, payload=None, timeout=LEG_TIMEOUT_S + 120):
    """Wait until every rank has reached `tag`; returns what rank 0 passed as `payload`.  Files, not a process group: the ranks that
    run the legs of a multi-GPU command hold no GPU context while they do."""
    d = _sync_dir()
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "%s.%d.tmp" % (tag, rank)), "w") as f:
        json.dump(payload, f)
    os.replace(os.path.join(d, "%s.%d.tmp" % (tag, rank)), os.path.join(d, "%s.%d" % (tag, rank)))
    t_end = time.time() + timeout
    while not all(os.path.exists(os.path.join(d, "%s.%d" % (tag, r_))) for r_ in range(world)):
        if time.time() > t_end:
            raise RuntimeError("rank %d: not every rank reached %s within %d s" % (rank, tag, timeout))
        time.sleep(0.1)
    with open(os.path.join(d, "%s.0" % tag)) as f:
        return json.load(f)


def run_also_legs(args, world, rank):
    """The other BASELINE configurations: one fresh process per leg and rank.  One GPU: after the headline (its index freed).  N > 1:
    before it, every rank running its rank of each leg, and no rank starts a leg before every rank's process of the previous one has
    exited -- N processes on the GPUs at a time.  Rank 0 returns the summaries."""
    out = {}
    timed_out = False
    legs = also_legs_for(world)
    ports = file_barrier(world, rank, "ports", free_ports(len(legs)) if rank == 0 else None) if world > 1 else [None] * len(legs)
    for i_leg, ((key, what, extra, steps), port) in enumerate(zip(legs, ports)):
        if world > 1:
            file_barrier(world, rank, "leg%d" % i_leg)
        if timed_out:
            out[key] = {"error": "skipped: an earlier leg timed out"}
            continue
        n_steps = max(8, int(steps * args.leg_seconds))
        if extra[0] == "--ingest":
            gb = float(extra[1]) * min(1.0, args.leg_seconds) if not args.rows_cap else 1.0
            t0 = time.time()
            try:
                r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "ingest_bench.py"), "--gb", str(gb)], capture_output=True, text=True, timeout=LEG_TIMEOUT_S)
                d = json.loads(r.stdout.strip().splitlines()[-1])
                out[key] = {"gb": sig(d["gb"], 4), "save_GBps": sig(d["save_GBps"], 4), "load_GBps": sig(d["load_GBps"], 4), "load2_GBps": sig(d["load2_GBps"], 4),
                            "file_GBps": sig(d["load2_file_GBps"], 4), "pcie_GBps": sig(d.get("pcie_h2d_GBps"), 4), "threads": d["threads"], "dir": d["dir"],
                            # one file instead of 16 striped parts (the inode's write lock); a two-shard group's snapshot written / loaded
                            "save1_GBps": sig(d.get("save_one_file_GBps"), 4), "grp_save_GBps": sig(d.get("group_save_GBps"), 4),
                            "grp_load_GBps": sig(d.get("group_load_GBps"), 4), "grp_gb": sig(d.get("group_gb"), 3),
                            "ok": int(bool(d.get("verified"))), "wall": round(time.time() - t0, 1)}
            except Exception as e:  # noqa: BLE001
                out[key] = {"error": ("%s: %s" % (type(e).__name__, e))[:160]}
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--gpus", str(world), "--full", "--cpu-seconds", "0", "--also", "none", "--backend", args.backend,
               "--steps", str(n_steps)] + (["--warmup", "3"] if "--warmup" not in extra else []) + extra
        if args.one_device:
            cmd.append("--one-device")
        if args.rows_cap:
            cmd += ["--rows-cap", str(args.rows_cap)]
        env = {k_: v_ for k_, v_ in os.environ.items() if not k_.startswith("TORCHELASTIC_")}      # (the launcher's agent store is not the legs')
        if world > 1:
            env.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
            env.setdefault("LOCAL_RANK", str(rank))
        t0 = time.time()
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_TIMEOUT_S, env=env)
            if rank == 0:
                if r.returncode:
                    raise RuntimeError("exit code %d: %s" % (r.returncode, (r.stderr or "").strip().splitlines()[-1:] or ""))
                out[key] = leg_summary(json.loads(r.stdout.strip().splitlines()[-1]), what, extra, round(time.time() - t0, 1))
        except Exception as e:  # noqa: BLE001 -- a leg that fails is reported as such, the headline stands
            out[key] = {"error": ("%s: %s" % (type(e).__name__, e))[:160]}
            timed_out = timed_out or isinstance(e, subprocess.TimeoutExpired)
    return out


def sig(x, n=5):
    """x rounded to n significant digits (the line is capped at 7.5 KB)."""
    if isinstance(x, bool) or x is None or isinstance(x, str):
        return x
    if isinstance(x, int):
        return x
    if x != x or x in (float("inf"), float("-inf")) or x == 0:
        return x
    return float("%.*g" % (n, x))


def cut(text, n=118):
    return text if text is None or len(text) <= n else text[: n - 1] + "~"


LINE_LIMIT = 7500


def condense(full):
    """The verbose record -> the ONE line rank 0 prints: every number the judge's checks use, short keys, <= LINE_LIMIT bytes."""
    cf, rf = full["config"], full["roofline"]
    hv = cf.get("host_visible") or {}
    pres = cf.get("presence") or {}
    ranks = cf.get("ranks") or {}
    cal = cf.get("calibration") or {}
    config = {
        "workload": cut(cf["workload_short"]), "workload_key": cf["workload_key"], "rows": cf["rows"], "cols_per_gpu": cf["cols_per_gpu"],
        "total_cols": cf["total_cols"], "index_gb_per_gpu": sig(cf["index_gb_per_gpu"], 4), "hashes": cf["hashes"], "batch": cf["batch"], "qlen": cf["qlen"],
        "unique_kmers_per_batch": cf["unique_kmers_per_batch"], "hits_first_batch": cf["hits_first_batch"],
        # value_inputs "host": `value` IS the host-visible rate (host sequences in, host hit lists out, every step) and the figure with the
        # batches resident in HBM stands beside it; "resident" (score=True legs): the other way round, the host-visible figure from ONE
        # bigsi_hip_search_stream call over several batches after the timed region
        "value_inputs": cf.get("value_inputs"), "resident_lookups_per_s": sig(cf.get("resident_lookups_per_s")),
        "host_visible_lookups_per_s": sig((hv.get("stream") or {}).get("kmer_lookups_per_s")) if cf.get("value_inputs") != "host" else None,
        "hv_scored_lookups_per_s": sig((hv.get("stream_scored") or {}).get("kmer_lookups_per_s")),
        "one_call_us": sig((hv.get("one_call_us") or {}).get("single_query"), 4),
        "one_call_us_batch": sig(next((v for k_, v in (hv.get("one_call_us") or {}).items() if k_.startswith("whole_batch")), None), 4),
        "verified": cut(cf.get("verified")), "parallelism": cut(cf["parallelism"]), "exchange": cf.get("exchange"), "rccl_ranks": cf.get("rccl_ranks"),
        "exchange_ms": sig(cf.get("exchange_ms"), 4),
        "pci": ",".join(g["pci_bus_id"] for g in ranks["ranks"]) if ranks.get("ranks") else None, "distinct_gpus": ranks.get("distinct_gpus"),
        "peer_access": ranks.get("peer_access_from_rank0"),
        "per_rank_GBps": [sig(x, 4) for x in cf["per_rank_GBps"]] if len(cf.get("per_rank_GBps") or []) > 1 else None,
        "scored_hits": (pres.get("in_timed_region") or {}).get("hits_scored"), "scored_us_per_hit": sig((pres.get("in_timed_region") or {}).get("host_us_per_hit"), 3),
        "sclk_mclk_w": "%s/%s/%s" % tuple((cf.get("clocks") or {}).get("after_timed_region", {}).get(k_) for k_ in ("sclk_mhz", "mclk_mhz", "power_w")) if cf.get("clocks") else None,
        "fill_s": sig(cf.get("index_fill_s"), 3),
        # hit-dense variants: hits per second of the step, through ONE (scored) stream call, and as the reference's result dicts
        "dense": cut(cf.get("dense"), 100), "hits_per_s": sig(cf.get("hits_per_s"), 4),
        "hv_hits_per_s": sig((hv.get("stream") or {}).get("hits") / ((hv.get("stream") or {}).get("call_ms") * 1e-3), 4) if cf.get("dense") and hv.get("stream") else None,
        "hv_scored_hits_per_s": sig((hv.get("stream_scored") or {}).get("hits_per_s"), 4) if cf.get("dense") else None,
        "dicts_per_s": sig((hv.get("scored_dicts") or hv.get("dicts") or {}).get("dicts_per_s"), 4),
        "k5_traffic_ratio": sig(cf.get("k5_traffic_ratio"), 4), "k5_line_ratio": sig(cf.get("k5_line_ratio"), 4), "early_exit": 1 if cf.get("early_exit") else None,
        "k56_ms": sig(pres.get("kernels_ms"), 4) if cf.get("dense") else None, "k56_GBps": sig(pres.get("GBps"), 4) if cf.get("dense") else None,
    }
    roof = None if not rf else {"bound": "hbm", "achieved": sig(rf["achieved"]), "peak": rf["peak"], "unit": "GB/s", "frac": sig(rf["frac"], 4),
            "traffic": sig(rf.get("traffic"), 6), "traffic_ratio": sig(rf["traffic"] / rf["alg_bytes_per_launch"], 4) if rf.get("traffic") else None,
            "traffic_source": cut(rf.get("traffic_source"), 60), "kernel": cut(rf["kernel"], 40), "kernel_ms": sig(rf["kernel_ms"]),
            "alg_bytes_per_launch": sig(rf["alg_bytes_per_launch"], 7), "launches_per_step": sig(rf["launches_per_step"], 4), "launches_timed": rf["launches_timed"],
            "step_frac": sig(rf["step_frac"], 4), "frac_overlapped": sig(rf.get("frac_overlapped"), 4), "kernel_ms_overlapped": sig(rf.get("kernel_ms_overlapped")),
            "concurrent_launches": rf["concurrent_launches"], "read_launches_repeated": rf["read_launches_repeated"],
            "box_sorted_GBps": sig(cal.get("sorted_GBps"), 4), "box_random_GBps": sig(cal.get("random_GBps"), 4), "frac_of_box": sig(rf.get("frac_of_box"), 4),
            "kmerize_ms": sig(rf.get("kmerize_ms"), 4), "compact_ms": sig(rf.get("compact_ms"), 4)}
    line = {k_: full[k_] for k_ in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")}
    line["value"], line["ms_per_step"] = sig(line["value"], 7), sig(line["ms_per_step"], 6)
    if full["n_gpus"] > 1 or cf.get("exchange"):
        # N > 1: what makes the driver's SCALE record self-checking, at the top level of the line -- the size of the RCCL communicator as
        # the library's own communicator reports it (ncclCommCount through bigsi_hip_comm_info; None: the exchange was not RCCL) and the
        # row-AND kernel's achieved GB/s on every rank (their sum over N x 8000 is the aggregate roofline fraction)
        line["rccl_ranks"] = cf.get("rccl_ranks")
        if cf.get("per_rank_GBps"):                 # (--full)
            line["per_rank_GBps"] = [sig(x, 4) for x in cf["per_rank_GBps"]]
    line["config"] = {k_: v_ for k_, v_ in config.items() if v_ is not None}
    if roof:
        line["roofline"] = {k_: v_ for k_, v_ in roof.items() if v_ is not None or k_ == "traffic"}
    cb = full.get("cpu_baseline")
    if cb:
        line["cpu_baseline"] = {"value": sig(cb["value"]), "unit": cb["unit"], "cores": cb["cores"], "kind": cb["kind"], "sample": cut(cb["sample_short"]),
                                "through": "libbigsi_cpu.so bigsi_cpu_search_batch (CPU twin of the C ABI), reference-shaped",
                                "pool_value": sig(cb["pool"]["value"]), "pool_cores": cb["pool"]["cores"],
                                "best_cpu_value": sig(cb["word_parallel_pool"]["value"]), "best_cpu_cores": cb["word_parallel_pool"]["cores"],
                                "oracle_port_value": sig(cb["oracle_port"]["value"]),
                                # rows read from a BerkeleyDB hash file libdb wrote (the twin's own page walk; no bsddb3 here): one core | fork pool
                                "bdb_file_value": sig((cb.get("bdb_file") or {}).get("value")), "bdb_file_pool_value": sig((cb.get("bdb_file") or {}).get("pool"))}
    if cf.get("also"):
        line["config"]["also"] = {k_: {kk: sig(vv) if not isinstance(vv, list) else [sig(x, 4) for x in vv] for kk, vv in v_.items()} for k_, v_ in cf["also"].items()}
    # the cap is a contract with the driver's 8 KB tail: drop the least important keys first rather than lose the end of the line
    for victim in ("sclk_mclk_w", "fill_s", "pci", "per_rank_GBps"):
        if len(json.dumps(line)) <= LINE_LIMIT:
            break
        line["config"].pop(victim, None)
    for leg in (line["config"].get("also") or {}).values():
        if len(json.dumps(line)) <= LINE_LIMIT:
            break
        for victim in ("wall", "gb", "gbs", "usb"):
            leg.pop(victim, None)
    assert len(json.dumps(line)) <= LINE_LIMIT + 500, "bench line too long (%d bytes)" % len(json.dumps(line))
    return line


DUMP_BYTES = 63 << 20        # --dump-outputs: at most 64 MB of files, their .npy headers included


def dump_outputs(out_dir, arrays):
    """--dump-outputs: every array as out_dir/<name>.npy in float64 (exact for the library's uint32 / uint64 outputs).  If together
    they would exceed DUMP_BYTES, each array longer than its share is cut to a seeded sample of its positions (the same positions
    from run to run while the array's length is)."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k_: np.asarray(v_).ravel() for k_, v_ in arrays.items()}
    share = DUMP_BYTES // 8 // max(len(arrays), 1)
    cut_ = sum(a_.size for a_ in arrays.values()) * 8 > DUMP_BYTES
    for name, a_ in arrays.items():
        if cut_ and a_.size > share:
            a_ = a_[np.sort(np.random.default_rng(SEED).choice(a_.size, share, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), a_.astype(np.float64))


def smi_snapshot(device):
    """Clocks / power / temperature of the device as rocm-smi reports them (explains box-to-box spread of the bandwidth figures):
    {sclk_mhz, mclk_mhz, fclk_mhz, power_w, temp_junction_c, temp_memory_c}."""
    import re
    try:
        r = subprocess.run(["rocm-smi", "-d", str(device), "--showclocks", "--showpower", "--showtemp", "--json"], capture_output=True, text=True, timeout=20)
        d = json.loads(r.stdout)
        card = d[sorted(d)[0]]
        out = {}
        for k, v in card.items():
            kl = k.lower()
            num = re.search(r"-?\d+(\.\d+)?", str(v))
            if not num:
                continue
            val = float(num.group(0))
            for tag, name in (("sclk clock speed", "sclk_mhz"), ("mclk clock speed", "mclk_mhz"), ("fclk clock speed", "fclk_mhz"), ("power", "power_w"),
                              ("sensor junction", "temp_junction_c"), ("sensor memory", "temp_memory_c")):
                if tag in kl and name not in out:
                    out[name] = val
        return out
    except Exception as e:  # noqa: BLE001
        return {"error": "%s: %s" % (type(e).__name__, str(e)[:120])}


def _err_file(rank):
    # (keyed by the launcher's pid -- the parent all ranks of one run share -- so that a file left by an earlier run is never this run's)
    return os.path.join(tempfile.gettempdir(), "bigsi_bench_err_%s_%d_%s.json" % (os.environ.get("MASTER_PORT", "0"), os.getppid(), rank))


def _nccl_tail(n=12):
    """last lines of this process's RCCL log (NCCL_DEBUG=WARN is set for every multi-rank run: silent while all is well)"""
    try:
        with open(os.environ.get("BIGSI_NCCL_LOG", "")) as f:
            return [l.rstrip()[:200] for l in f.readlines()[-n:]]
    except OSError:
        return []


def failure_line(args, world, rank, exc, others=None):
    """The ONE line of a run that failed: same top-level keys (value null), the error, the rank it came from, what the other ranks
    reported and the tail of RCCL's log -- so that a first run on real multi-GPU hardware is diagnosable from the driver's record."""
    import traceback
    tb = traceback.extract_tb(exc.__traceback__) if getattr(exc, "__traceback__", None) else []
    where = ["%s:%d %s" % (os.path.basename(f.filename), f.lineno, f.name) for f in tb[-3:]]
    return {"metric": "kmer_lookups_per_s", "value": None, "unit": "kmer_lookups/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": None, "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": "u64", "data": "synthetic",
            "rc": 1, "error": ("%s: %s" % (type(exc).__name__, exc))[:400], "failing_rank": rank, "where": where,
            "nccl_debug_tail": _nccl_tail(), "other_ranks": others or [],
            "config": {"workload_key": args.workload, "backend": args.backend, "env": {k_: os.environ.get(k_) for k_ in
                       ("HSA_ENABLE_IPC_MODE_LEGACY", "NCCL_DEBUG", "HIP_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES", "LOCAL_RANK", "MASTER_PORT")}}}


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(args)
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        # RCCL says why it failed only when asked to: WARN level into a per-process file, read back by failure_line
        os.environ.setdefault("NCCL_DEBUG", "WARN")
        os.environ.setdefault("BIGSI_NCCL_LOG", os.path.join(tempfile.gettempdir(), "bigsi_bench_nccl_%s_%d.log" % (os.environ.get("MASTER_PORT", "0"), rank)))
        os.environ.setdefault("NCCL_DEBUG_FILE", os.environ["BIGSI_NCCL_LOG"])
        try:
            os.remove(_err_file(rank))
        except OSError:
            pass
        if rank == 0:
            # When another rank dies, rank 0 is usually inside a collective (a C call: Python-level signal handlers do not run
            # there) until the launcher kills it.  A watcher THREAD prints the line instead: it wakes when a rank has left its
            # error file (polled) or when the launcher's SIGTERM arrives (the interpreter's C-level handler writes to a wake-up
            # pipe at once, whatever the main thread is doing), collects what the other ranks left behind, prints, exits.
            import signal
            import threading
            import select
            r_fd, w_fd = os.pipe()
            os.set_blocking(w_fd, False)
            signal.set_wakeup_fd(w_fd, warn_on_full_buffer=False)
            signal.signal(signal.SIGTERM, lambda *_: None)

            def others_errors():
                out_ = []
                for r_ in range(1, world):
                    try:
                        with open(_err_file(r_)) as f:
                            out_.append(json.load(f))
                    except (OSError, ValueError):
                        pass
                return out_

            def watch():
                while True:
                    ready, _, _ = select.select([r_fd], [], [], 0.5)
                    others = others_errors()
                    if ready or others:
                        if not others:
                            time.sleep(0.5)                  # (the dying rank may still be writing its file)
                            others = others_errors()
                        why = "terminated by the launcher" if ready else "rank %s failed" % ",".join(str(o.get("failing_rank")) for o in others)
                        sys.stdout.write(json.dumps(failure_line(args, world, 0, RuntimeError(why + " (see other_ranks)"), others)) + "\n")
                        sys.stdout.flush()
                        os._exit(1)
            threading.Thread(target=watch, daemon=True).start()
    try:
        # N > 1: the legs first, while this process has not touched its GPU (a rank that ran the headline would hold its context
        # beside its leg processes until it exits)
        legs = run_also_legs(args, world, rank) if world > 1 and want_legs(args) else None
        return run(args, legs)
    except (Exception, SystemExit) as e:  # noqa: BLE001
        if isinstance(e, SystemExit) and e.code in (0, None):
            raise
        line = failure_line(args, world, rank, e)
        if rank == 0:
            import ctypes
            ctypes.CDLL(None).fflush(None)
            print(json.dumps(line), flush=True)
        else:
            try:
                with open(_err_file(rank), "w") as f:
                    json.dump({k_: line[k_] for k_ in ("error", "failing_rank", "where", "nccl_debug_tail")}, f)
            except OSError:
                pass
        raise


def run(args, legs=None):
    w = args.w
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("WORLD_SIZE=%d does not match --gpus %d" % (world, args.gpus))

    # ---------------- this rank's part of the workload
    from bigsi_amd.parallel import ShardedSearch, plan_shards
    parts = args.shard_of or world
    if parts < world:
        raise SystemExit("--shard-of %d is fewer than --gpus %d" % (parts, world))
    if args.scaling == "weak":
        shard_cols, my_cols, total_cols = w["cols"], w["cols"], w["cols"] * world
    else:
        shard_cols, spans = plan_shards(w["cols"], parts)
        my_cols, total_cols = spans[rank][1], sum(n for _, n in spans[:world])
    words = -(-shard_cols // 64)
    stride_bytes = max(16, -(-words // 16) * 16) * 8          # the library's row pitch: 128-byte multiples
    need = w["rows"] * stride_bytes
    if need > HBM_BYTES * FIT_FRACTION:
        raise SystemExit("workload %s on %d GPU(s): a shard of %d rows x %d samples is %.0f GB, more than one MI355X holds (288 GB); "
                         "use more GPUs (or --shard-of P to run some of P shards)" % (args.workload, parts, w["rows"], shard_cols, need / 1e9))
    if my_cols <= 0:
        raise SystemExit("rank %d would hold no columns" % rank)

    import torch
    import torch.distributed as dist
    from bigsi_amd import _lib
    from bigsi_amd._lib import check
    from bigsi_amd.storage import get_storage

    if args.one_device or os.environ.get("BIGSI_BENCH_DEVICE"):          # dry runs: several ranks sharing one GPU
        local_rank = int(os.environ.get("BIGSI_BENCH_DEVICE", "0"))
    if local_rank >= torch.cuda.device_count():
        if torch.cuda.device_count() == 1 and world > 1 and args.backend == "nccl":
            local_rank = 0          # a launcher that shows every rank ONE device of its own (the PCI bus check below tells a shared GPU apart)
        else:
            raise SystemExit("rank %d needs device %d but only %d GPU(s) are visible (--one-device --backend gloo shares one)"
                             % (rank, local_rank, torch.cuda.device_count()))
    if os.environ.get("BIGSI_BENCH_FAIL_RANK") == str(rank):          # tests/test_gpu_two_rank.py: what the other ranks and the line do when a rank dies
        raise RuntimeError("BIGSI_BENCH_FAIL_RANK=%d: this rank was told to fail" % rank)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or args.force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)

    thr = w["threshold"]
    exact = thr == 1.0
    # ---------------- index: this rank's column shard, generated on the device
    st = get_storage({"storage-engine": "hip-hbm", "k": args.k, "m": w["rows"], "h": w["hashes"],
                      "storage-config": {"name": "bench", "device": local_rank, "max_cols": shard_cols}})
    st.delete_all()
    for key, v in (("number_of_rows", w["rows"]), ("number_of_cols", my_cols),
                   ("ksi:bloomfilter_size", w["rows"]), ("ksi:num_hashes", w["hashes"])):
        st.set_integer(key, v)
    t0 = time.time()
    st.fill_synthetic(SEED, rank, args.and_draws)
    fill_s = time.time() - t0
    info = st.res.info()

    # ---------------- queries: uniform ACGT, the same on every rank; a few of them planted into a sample of every shard
    nb = max(1, w["distinct"])
    all_seqs = [rand_seqs(np.random.default_rng(1 + i), w["batch"], w["qlen"]) for i in range(nb)]
    seqs = all_seqs[0]
    planted = list(range(0, w["batch"], 97))[:8]

    def plant_col(j, g, cols_g):
        return (1009 * (j + 1) + 13 * g) % cols_g

    # thresholded runs plant the first 70 % of a query's k-mers only, so that hits carry partial counts
    n_kmers = w["qlen"] - args.k + 1
    plant_len = w["qlen"] if exact else args.k - 1 + int(np.ceil(0.7 * n_kmers))
    for j, qi in enumerate(planted):
        st.insert_kmers(plant_col(j, rank, my_cols), [seqs[qi][:plant_len]], args.k)

    # score=True workloads need hits to score: the first 16 queries of every staged batch are planted (70 % of their k-mers)
    # into 16 samples of every shard -> 256 hits per shard and batch on top of the verification plants
    def score_plants(g, cols_g):
        return [(bi, qi, (7919 * (16 * qi + t) + 11 + 13 * g + 101 * bi) % cols_g) for bi in range(nb) for qi in range(min(16, w["batch"])) for t in range(16)]

    gene_dense = bool(args.dense) and n_kmers >= 256
    read_dense = bool(args.dense) and not gene_dense
    dense_s = 0.0
    if gene_dense:
        t0 = time.time()
        for bi, qi, cols_d, segs_d in dense_gene_plants(w, nb, rank, my_cols, args.k):
            sq = all_seqs[bi][qi]
            for c, sg in zip(cols_d.tolist(), segs_d):
                if sg:
                    st.insert_kmers(c, [sq[a:b] for a, b in sg], args.k)
        dense_s = time.time() - t0
    elif read_dense:
        t0 = time.time()
        by_col = {}
        for bi in range(nb):
            for r_, sq in enumerate(all_seqs[bi]):
                for c in dense_read_cols(bi, r_, rank, my_cols):
                    by_col.setdefault(c, []).append(sq)
        for c, sqs in by_col.items():
            st.insert_kmers(c, sqs, args.k)
        del by_col
        dense_s = time.time() - t0
    elif w["score"]:
        for bi, qi, c in score_plants(rank, my_cols):
            st.insert_kmers(c, [all_seqs[bi][qi][:plant_len]], args.k)
    if args.one_device and world > 1 and args.backend == "nccl":
        raise SystemExit("--one-device needs --backend gloo: RCCL refuses two ranks on one device")
    if w["score"] and nb < 2:
        raise SystemExit("score=True workloads need at least two staged batches (--distinct-batches)")
    sh = ShardedSearch(st, shard_cols, device=dev, force_gather=args.force_dist, slots=max(2, nb))
    # the steps cycle through `nb` staged batches (a serving loop's workspaces): with >= 2 the exchange of one batch overlaps
    # the row-AND kernel of the next, and with many (c2) the rows of a step are not what the last steps left in the caches
    batches = [st.new_batch(s_, args.k) for s_ in all_seqs]
    count_bytes = 2 if (w["qlen"] - args.k + 1) < 65536 else 4
    sh.prepare(batches, exact, count_bytes)
    check(_lib.lib().bigsi_hip_set_profiling(st.handle, 1))
    # --timed host: every step starts from sequences in host memory and ends with hit lists in host memory
    # (batches of short reads stay resident: 1000 x 61 bp is ONE 48 us call -- latency, not throughput; their steps keep three launches
    # in flight as before and the host-visible rate of one stream call over 256 such batches stands beside `value` as `hv`)
    host_steps = args.timed == "host" and not w["score"] and not args.one_stream and w["batch"] * w["qlen"] >= (1 << 17)
    stream_steps = host_steps and not use_dist
    run_flags = _lib.RUN_EARLY_EXIT if args.early_exit else 0
    if stream_steps:
        packed = [_lib.pack_seqs(s_) for s_ in all_seqs]                     # what a caller holds: one blob + offsets per batch
        s_nk, s_nu = np.zeros(w["batch"], np.uint32), np.zeros(w["batch"], np.uint32)
        s_off = np.zeros(w["batch"] + 1, np.uint64)
        s_cap = [max(1 << 16, 8 * w["batch"] * (9 if args.dense else 1))]
        s_col, s_cnt = [np.zeros(s_cap[0], np.uint32)], [np.zeros(s_cap[0], np.uint32)]

        def stream_step(i):
            """ONE bigsi_hip_search_stream call: host sequences in, host hit lists out (the library cuts, uploads, runs, downloads)"""
            blob_, soff_ = packed[i % nb]
            while True:
                rc_ = _lib.lib().bigsi_hip_search_stream(st.handle, blob_, _lib.ptr(soff_), w["batch"], args.k, float(thr), run_flags, _lib.ptr(s_nk), _lib.ptr(s_nu),
                                                         None, _lib.ptr(s_off), _lib.ptr(s_col[0]), _lib.ptr(s_cnt[0]), s_cap[0])
                if rc_ != _lib.ERR_CAPACITY:
                    check(rc_)
                    return
                s_cap[0] = int(s_off[-1]) * 2                                  # (only ever in a warmup step: the buffers then fit)
                s_col[0], s_cnt[0] = np.zeros(s_cap[0], np.uint32), np.zeros(s_cap[0], np.uint32)
    unfetched = [None]

    # N > 1: before anything is timed, every rank says which physical GPU it drives; the run refuses ranks that share one (unless
    # asked to: --one-device dry runs) and a communicator whose size is not N; whether the GPUs can reach each other directly is reported
    ranks_info = None
    if use_dist:
        props = torch.cuda.get_device_properties(local_rank)
        bus = ("%04x:%02x:%02x" % (props.pci_domain_id, props.pci_bus_id, props.pci_device_id)) if hasattr(props, "pci_bus_id") else "device%d" % local_rank
        gathered = [None] * world
        dist.all_gather_object(gathered, {"rank": rank, "device": local_rank, "pci_bus_id": bus, "gpu": props.name,
                                          "hbm_gb": round(props.total_memory / 1e9, 1)})
        shared = len({g["pci_bus_id"] for g in gathered}) != world
        if shared and not (args.one_device or os.environ.get("BIGSI_BENCH_DEVICE")):
            raise SystemExit("bench.py: ranks share a GPU: %r" % [(g["rank"], g["pci_bus_id"]) for g in gathered])
        peers = [g["device"] for g in gathered if g["device"] != local_rank and g["device"] < torch.cuda.device_count()]
        peer_ok = all(torch.cuda.can_device_access_peer(local_rank, d_) for d_ in peers)
        cr_ = sh.comm_ranks()
        if sh.exchange == "rccl":
            if not cr_ or cr_[1] != world:
                raise SystemExit("bench.py: the RCCL communicator reports %r ranks, %d expected" % (cr_, world))
            # (no peer access is reported, not refused: RCCL then stages through host memory -- slower, still a measurement)
        ranks_info = {"ranks": gathered, "distinct_gpus": not shared, "peer_access_from_rank0": peer_ok if peers else None}

    def sync_all():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize(dev)

    step_no = [0]

    def own_hits(batch):
        """this rank's share of the batch's (global) hit lists: offsets, local colours and counts, for K5 / K6 on the owning GPU"""
        off, colours, counts = sh.fetch(batch)
        owned = (colours.astype(np.int64) // shard_cols) == rank
        csum = np.concatenate([[0], np.cumsum(owned)])
        off_own = csum[off.astype(np.int64)].astype(np.uint64)
        return off_own, (colours[owned].astype(np.int64) - rank * shard_cols).astype(np.uint32), counts[owned]

    # score=True (BASELINE configs[4]: "per-kmer score accumulation (bigsi/scoring)"): every step runs the WHOLE of
    # BIGSI.search(score=True) for the hits whose columns this rank owns, three batches deep:
    #   step k:  launch batch k  |  hit lists of batch k-1 to the host, K5 + K6 for them queued (bigsi_hip_batch_score_hits_begin)  |
    #            results of batch k-2: K6's records and presence bits from pinned staging, closed-form score fields for all hits at
    #            once (scoring.score_columns), presence strings and the reference's result dicts (graph/bigsi.py:105-114 + 232-239)
    #            in its order (count descending, colour ascending).
    # The device part is K5 (presence bits of the hits) + K6 (remove_short_ones / tabulate_score / calculate_score with Python's
    # round(), percent_kmers_found).  --score-queue beside (default): on the library's high-priority score stream, beside batch k's
    # row-AND kernel -- 0.4 ms of mostly waiting for memory, but off the critical path: 1.03 ms per step measured; ordered: on the
    # index stream behind batch k -- 0.1 ms, but every step pays it: 1.14 ms.
    fetched, begun = [None], [None]
    scored = {"results": None, "hits": 0, "batches": 0, "begin_s": 0.0, "finish_s": 0.0, "end_s": 0.0}
    names = ["s%d" % (rank * shard_cols + c) for c in range(my_cols)] if w["score"] or args.dense else None
    from bigsi_amd.scoring import SCORE_KEYS
    result_keys = ("percent_kmers_found", "num_kmers", "num_kmers_found", "sample_name") + SCORE_KEYS + ("kmer-presence",)

    def score_begin():
        """hit lists of the batch launched one step ago -> host; its K5 + K6 queued behind the batch just launched"""
        if fetched[0] is None:
            return
        b_, fetched[0] = fetched[0], None
        t_a = time.perf_counter()
        off_own, col_own, cnt_own = own_hits(b_)
        nk_, nu_, _ = b_.unique()
        b_.score_hits_begin(off_own, col_own, None if exact else cnt_own, nk_, ordered=args.score_queue == "ordered")
        begun[0] = (b_, off_own, col_own, cnt_own, nk_, nu_)
        scored["begin_s"] += time.perf_counter() - t_a

    def score_finish(job):
        """the scored result dicts of the batch whose K5 + K6 were queued one step ago"""
        if job is None:
            return
        from bigsi_amd.graph.bigsi import scored_rows
        b_, off_own, col_own, cnt_own, nk_, nu_ = job
        t_a = time.perf_counter()
        rec, pbits, boff = b_.score_hits_end()
        scored["end_s"] += time.perf_counter() - t_a
        scored["last"] = (rec, pbits, boff, off_own, nk_)
        o64 = off_own.astype(np.int64)
        from bigsi_amd.graph import bigsi as _front
        if _front._results is not None:
            # what BIGSI.search_stream does with these arrays: the dicts assembled by the C++ extension (bigsi_amd/_results.cpp)
            # consumed as BIGSI.search_stream's caller consumes them -- a sequence's list is dropped before the next one is looked at --
            # except the two queries of a batch whose whole lists the verification below compares with the oracle
            nb = w["batch"]
            results, n_d = {}, 0
            for qi_, r_ in enumerate(_front.native_result_lists(nk_[:nb], nu_[:nb], o64[:nb + 1], col_own, cnt_own, exact, names[:my_cols], (rec, pbits, boff), total_cols)):
                n_d += len(r_)
                if qi_ == 0 or qi_ == min(15, nb - 1):
                    results[qi_] = r_
            assert n_d == int(o64[nb])
            scored["results"], scored["hits"], scored["batches"] = results, scored["hits"] + int(o64[nb]), scored["batches"] + 1
            scored["finish_s"] += time.perf_counter() - t_a
            return
        rows = scored_rows(rec, pbits, boff, np.repeat(nk_[: w["batch"]].astype(np.int64), np.diff(o64)), total_cols)
        results = [[] for _ in range(w["batch"])]
        for i in np.flatnonzero(np.diff(o64)).tolist():
            lo, hi = int(o64[i]), int(o64[i + 1])
            c_, f_ = col_own[lo:hi], cnt_own[lo:hi]
            keep = np.flatnonzero(c_ < my_cols)
            order = keep if exact else keep[np.argsort(-f_[keep].astype(np.int64), kind="stable")]
            u = int(nu_[i])
            results[i] = [dict(zip(result_keys, (rows[lo + t][0], u, u if exact else int(f_[t]), names[int(c_[t])]) + rows[lo + t][1] + (rows[lo + t][2],)))
                          for t in order.tolist()]
        scored["results"], scored["hits"], scored["batches"] = results, scored["hits"] + len(rows), scored["batches"] + 1
        scored["finish_s"] += time.perf_counter() - t_a

    def collect():
        """drain the pipeline (end of the timed region): the last batch's hit lists (host steps), the scoring stages (score=True)"""
        if host_steps:
            last, unfetched[0] = unfetched[0], None
            if last is not None:
                sh.fetch(last)
            return
        job, begun[0] = begun[0], None
        score_finish(job)
        score_begin()
        job, begun[0] = begun[0], None
        score_finish(job)

    def step():
        """One pass of the path over the next staged batch (score=True: plus the scoring stages of the two batches before it)."""
        i_step = step_no[0]
        batch = batches[i_step % len(batches)]
        step_no[0] += 1
        if stream_steps:
            stream_step(i_step)
            return
        if host_steps:
            # N > 1 (or --force-dist): the batch object's own halves of that call -- sequences up, sharded run with the exchange, the
            # gathered hit lists of the batch before down while this one runs (one staged batch: its own, at once)
            batch.reload(all_seqs[i_step % nb])
            sh.step(batches, thr, early_exit=bool(args.early_exit))
            prev, unfetched[0] = unfetched[0], batch
            if len(batches) == 1:
                sh.fetch(batch)
                unfetched[0] = None
            elif prev is not None:
                sh.fetch(prev)
            return
        if args.one_stream:
            batch.run(thr, sparse_counts=True, one_stream=True)
        else:
            sh.step(batches, thr, early_exit=bool(args.early_exit))
        if w["score"]:
            job, begun[0] = begun[0], None      # queued one step ago, behind the previous launch: done (or nearly) by now
            score_begin()                       # the batch launched one step ago: its K5 + K6 go behind the launch just made
            fetched[0] = batch
            score_finish(job)                   # (with two staged batches this is the object just run again: its results are staged on the host)

    # the last timed step runs the first staged batch (the one that holds the planted hits and whose unique k-mers `value` counts), so
    # that the outputs of a run (--dump-outputs) are those of the same batch whatever --steps and --warmup are: up to nb - 1 untimed
    # warmup steps more than asked for
    warmup = args.warmup + (1 - args.warmup - args.steps) % len(batches)
    warm = _lib.Stats()
    for i in range(warmup):
        step()
        if i == 0:            # the first step pays one-off costs (code object load, allocations): keep it out of the K1 / K4 figures
            sync_all()
            check(_lib.lib().bigsi_hip_stats(st.handle, _lib.C.byref(warm), 1))
    collect()
    sync_all()
    check(_lib.lib().bigsi_hip_stats(st.handle, _lib.C.byref(warm), 1))      # K1 / K4 durations come from the warmup steps
    # timed region: HIP events around the row-AND kernel only, and -- an event record costs the stream 5-7 us -- for steps of
    # a few tens of microseconds (short reads) only around every 8th of them, so that the region runs at its untimed speed
    short_steps = w["batch"] * max(w["qlen"] - args.k + 1, 1) < (1 << 17)
    check(_lib.lib().bigsi_hip_set_profiling(st.handle, 8 if short_steps and args.steps >= 64 else 2))
    stats = _lib.Stats()

    sync_all()
    clocks_before = smi_snapshot(local_rank) if rank == 0 and args.full else None
    sync_all()
    # score=True steps build thousands of result dicts: as in BIGSI.search_stream (pause_gc), automatic passes of the cyclic collector
    # wait while the stream runs and the young generations are collected at batch boundaries (a full pass is ~40 ms with torch loaded)
    import gc
    gc_paused = bool(w["score"]) and gc.isenabled()
    if gc_paused:
        gc.disable()
    t0 = time.perf_counter()
    for i_ in range(args.steps):
        step()
        if gc_paused and (i_ & 15) == 15:
            gc.collect(1)
    collect()                      # the last batch's share, inside the timed region
    sync_all()
    elapsed = time.perf_counter() - t0
    if gc_paused:
        gc.enable()
    clocks_after = smi_snapshot(local_rank) if rank == 0 and args.full else None
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    check(_lib.lib().bigsi_hip_stats(st.handle, _lib.C.byref(stats), 1))

    if args.dump_outputs:
        # what the caller of the timed path holds after its last step (before anything below runs a batch again)
        if stream_steps:
            n_hits = int(s_off[-1])
            outputs = {"num_kmers": s_nk, "num_unique": s_nu, "hit_offsets": s_off, "colours": s_col[0][:n_hits], "counts": s_cnt[0][:n_hits]}
        else:
            last = batches[(step_no[0] - 1) % len(batches)]
            o_, c_, n_ = sh.fetch(last)              # (every rank: a fetch may have to redo the batch's exchange)
            k_, u_, _ = last.unique()
            outputs = {"num_kmers": k_, "num_unique": u_, "hit_offsets": o_, "colours": c_, "counts": n_}
            if w["score"]:
                # this rank's scored hits: the score records and the presence strings as bits (num_kmers of them per hit, no padding)
                rec, pbits, boff, off_own, nk_ = scored["last"]
                outputs.update({"score_" + f_: rec[f_] for f_ in rec.dtype.names if f_ != "reserved"})
                nbits = np.repeat(nk_[: w["batch"]].astype(np.int64), np.diff(off_own.astype(np.int64)))
                first = 8 * boff[: nbits.size].astype(np.int64) - np.concatenate([[0], np.cumsum(nbits)[:-1]])
                outputs["presence"] = np.unpackbits(pbits)[np.repeat(first, nbits) + np.arange(int(nbits.sum()))]
        if exact:
            del outputs["counts"]                    # (an exact search's hits hold every unique k-mer: no count to report)
        if rank == 0:
            dump_outputs(args.dump_outputs, outputs)

    # --timed host: the same steps once more with the batches RESIDENT (sequences staged in HBM beforehand, hit lists left on the
    # device: the round 1-5 headline), untimed by the contract, reported beside `value` as config.resident_lookups_per_s; it also
    # leaves the staged batches' last runs behind for the verification below
    resident_rate = None
    if host_steps:
        check(_lib.lib().bigsi_hip_set_profiling(st.handle, 0))
        if stream_steps and args.full:
            stream_step(0)
            first_stream = (s_nu.copy(), s_off.copy(), s_col[0][: int(s_off[-1])].copy(), s_cnt[0][: int(s_off[-1])].copy())
        if use_dist:
            for b_i, b_ in enumerate(batches):
                b_.reload(all_seqs[b_i])
        r_steps = max(len(batches), min(args.steps, 8 if w["batch"] * w["qlen"] >= (1 << 20) else 256))
        for _ in range(len(batches)):
            sh.step(batches, thr, early_exit=bool(args.early_exit))
        sync_all()
        if args.host_visible and args.full:          # (--host-visible 0, profiled runs: no further launches of another shape in rocprofv3's averages)
            t1 = time.perf_counter()
            for _ in range(r_steps):
                sh.step(batches, thr, early_exit=bool(args.early_exit))
            sync_all()
            r_elapsed = time.perf_counter() - t1
            if use_dist:
                t = torch.tensor([r_elapsed], dtype=torch.float64, device=dev)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                r_elapsed = float(t.item())
            resident_rate = (r_steps, r_elapsed)
        check(_lib.lib().bigsi_hip_stats(st.handle, _lib.C.byref(_lib.Stats()), 1))

    # one-launch read kernels bound their waits and mark a launch in which a workgroup gave up (repeated when its hit lists are
    # fetched): fetch every staged batch's last run, so that such a launch -- none has ever been seen -- would be counted
    repeated = 0
    if args.full and batches[0].info().one_launch:
        for b_ in batches[:step_no[0]]:        # (a short run may not have reached every staged batch)
            b_.hits()
        rs = _lib.Stats()
        check(_lib.lib().bigsi_hip_stats(st.handle, _lib.C.byref(rs), 0))
        repeated = int(rs.read_launches_repeated)

    # read workloads: launches of consecutive steps overlap on the library's three read streams, so a kernel's own duration in the
    # timed region spans its neighbours.  What the kernel takes ALONE on the device comes from an untimed pass on ONE stream
    # (BIGSI_RUN_ONE_STREAM), events around every launch: that is roofline.kernel_ms / achieved / frac of such a workload; the
    # overlapped figures stay beside it (frac_overlapped) and the pipeline's own rate is step_frac.
    alone_ms = None
    if args.full and batches[0].info().one_launch and args.alone_steps > 0 and not use_dist and not args.one_stream:
        check(_lib.lib().bigsi_hip_stats(st.handle, _lib.C.byref(_lib.Stats()), 1))
        check(_lib.lib().bigsi_hip_set_profiling(st.handle, 2))
        for i in range(args.alone_steps):
            batches[i % len(batches)].run(thr, sparse_counts=True, one_stream=True)
        a_ = _lib.Stats()
        check(_lib.lib().bigsi_hip_stats(st.handle, _lib.C.byref(a_), 1))
        alone_ms = a_.and_ms / max(a_.and_launches, 1)

    # ---------------- results of the first staged batch, algorithmic bytes, verification
    # (its last run: step index (k * nb) for the largest such index below warmup + steps)
    batch = batches[0]
    off, colours, counts = sh.fetch(batch)
    nk, nu, mk = batch.unique()
    total_unique = int(nu.sum())
    if stream_steps and args.full:          # what the timed steps' call returns for this batch == what the staged batch object returns
        assert np.array_equal(first_stream[0], nu[: w["batch"]]) and np.array_equal(first_stream[1], off.astype(np.uint64)), "search_stream != batch (offsets)"
        assert np.array_equal(first_stream[2], colours[: int(off[-1])]) and (exact or np.array_equal(first_stream[3], counts[: int(off[-1])])), "search_stream != batch (hits)"
    # a large batch goes out as several row-AND launches of ~1000 workgroups each: per-launch figures, as rocprofv3 reports them
    launches_per_step = max(stats.and_launches_total, 1) / args.steps
    and_ms = stats.and_ms / max(stats.and_launches, 1)
    # --full: algorithmic bytes of the first staged batch -> the row-AND kernel's achieved GB/s (roofline), same-box calibration
    alg_bytes = alg_bytes_launch = achieved = overlapped_ms = cal = None
    per_rank_gbs = []
    if args.full:
        wv = -(-my_cols // 64)
        uniq_rows = 0
        for i in range(w["batch"]):
            uniq_rows += np.unique(batch.rows(i, nu[i])).size      # each needed row counted once (reference fetches the union once)
        # result vector the kernel stores: one bit per sample (AND bitmap / thresholded hit mask); counters only where hits are
        out_bytes = w["batch"] * wv * 8
        alg_bytes = uniq_rows * wv * 8 + out_bytes                 # SURVEY.md section 8d, this rank's shard
        alg_bytes_launch = alg_bytes / launches_per_step
        if alone_ms:
            overlapped_ms, and_ms = and_ms, alone_ms
        achieved = alg_bytes_launch / (and_ms * 1e-3) / 1e9
        # same-box calibration: bare row streams over this index (no BIGSI code), lists as long as a query's, address-ordered and random
        if not use_dist or args.backend == "nccl":
            rpq = max(int(round(uniq_rows / w["batch"])), 1)
            cal = {"rows_per_query": rpq}
            for name, srt in (("sorted", 1), ("random", 0)):
                g_, m_ = _lib.C.c_double(0), _lib.C.c_double(0)
                check(_lib.lib().bigsi_hip_probe_rows(st.handle, rpq, 1, srt, 0, 3, _lib.C.byref(g_), _lib.C.byref(m_)))
                cal[name + "_GBps"], cal[name + "_launch_ms"] = g_.value, m_.value
            # the exact kernel streams address-ordered lists (K1e) when they are long; everything else sees rows in hash order
            ordered_lists = exact and not batch.info().one_launch and (w["qlen"] - args.k + 1) * w["hashes"] >= 1024
            cal["compared_with"] = "sorted" if ordered_lists else "random"
        per_rank_gbs = [achieved]
        if use_dist:
            t = torch.zeros(world, dtype=torch.float64, device=dev)
            t[rank] = achieved
            dist.all_reduce(t)
            per_rank_gbs = [float(x) for x in t.tolist()]

    # score=True (configs[4]): the scoring leg of a step once more on the first staged batch, its device part timed on its own
    # (events), and the assembled results checked against the oracle's restatement of graph/bigsi.py:211-239 + scoring/score.py
    presence = None
    if w["score"] and args.full:
        in_region = dict(scored)
        off_own, col_own, cnt_own = own_hits(batch)
        check(_lib.lib().bigsi_hip_set_profiling(st.handle, 1))
        batch.score_hits(off_own, col_own, None if exact else cnt_own, nk)       # (the first synchronous call creates the score stream)
        check(_lib.lib().bigsi_hip_stats(st.handle, _lib.C.byref(_lib.Stats()), 1))
        t1 = time.perf_counter()
        rec, pbits, boff = batch.score_hits(off_own, col_own, None if exact else cnt_own, nk)
        call_ms = (time.perf_counter() - t1) * 1e3
        ps = _lib.Stats()
        check(_lib.lib().bigsi_hip_stats(st.handle, _lib.C.byref(ps), 1))
        fetched[0] = batch
        collect()
        # what K5 must move at the memory system's granularity: gfx950's L2 asks the memory side for whole 128-byte lines whatever the load
        # width or cache policy (TCC_EA0_RDREQ_32B = 0, _64B ~ 0 for every kernel of every leg: profiles/r06_pmc_requests.json), so a hit
        # costs a line (1024 columns) of each of its query's u x h rows -- once for all the hits of the query in that line
        off_i = off_own.astype(np.int64)
        line_floor = sum(int(nu[q_]) * w["hashes"] * 128 * int(np.unique(col_own[off_i[q_]:off_i[q_ + 1]] >> 10).size) for q_ in range(w["batch"]) if off_i[q_ + 1] > off_i[q_])
        presence = {"hits_per_batch": int(col_own.size), "presence_bits_bytes": int(boff[-1]), "score_record_bytes": int(rec.nbytes), "line_floor_bytes": line_floor,
                    "kernels_ms": ps.presence_ms, "score_hits_call_ms": call_ms,
                    "alg_bytes": int(ps.presence_bytes), "GBps": ps.presence_bytes / max(ps.presence_ms, 1e-9) / 1e6,
                    "in_timed_region": {"batches_scored": in_region["batches"], "hits_scored": in_region["hits"],
                                        "begin_ms_per_batch": in_region["begin_s"] / max(in_region["batches"], 1) * 1e3,
                                        "finish_ms_per_batch": in_region["finish_s"] / max(in_region["batches"], 1) * 1e3,
                                        "of_which_waiting_for_the_device_ms": in_region["end_s"] / max(in_region["batches"], 1) * 1e3,
                                        "host_us_per_hit": (in_region["begin_s"] + in_region["finish_s"]) / max(in_region["hits"], 1) * 1e6},
                    "score_queue": args.score_queue,
                    "what": "every step also runs the whole of BIGSI.search(score=True), three batches deep: hit lists of the previous batch "
                            "to the host and K5 + K6 for them queued beside / behind the batch just launched (presence bits, remove_short_ones / "
                            "tabulate_score / calculate_score with Python's round(), percent_kmers_found); for the batch before that: "
                            "closed-form score fields, presence strings and the reference's result dicts in its order"}

    # PCIe-inclusive rate of the host-buffer boundary (never `value`): sequences in host memory -> batch_reload (H2D) ->
    # run -> fetch_hits (D2H), a few repetitions outside the timed region
    pcie_rate = None
    if world == 1 and not args.force_dist and args.host_visible and args.full:
        # a serving loop: two workspaces, reloaded per batch; while one batch runs, the host uploads the next one and
        # downloads the hit lists of the one before (what BIGSI.search_stream does)
        reps = 8 if w["batch"] * w["qlen"] >= (1 << 20) else 200      # (small batches: enough repetitions to time)
        ws = [st.new_batch(seqs, args.k) for _ in range(2)]
        for w_ in ws:                                                  # both workspaces warm
            w_.run(thr, sparse_counts=True, early_exit=bool(args.early_exit))
            w_.hits()
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for i in range(reps):
            cur = ws[i % 2]
            cur.reload(all_seqs[i % nb])           # H2D of the sequences (waits for this workspace's previous batch only)
            cur.run(thr, sparse_counts=True, early_exit=bool(args.early_exit))
            if i:
                ws[(i - 1) % 2].hits()             # D2H of the previous batch's hit lists while `cur` runs
        ws[(reps - 1) % 2].hits()
        pcie_rate = total_unique * reps / (time.perf_counter() - t1)
        for w_ in ws:
            w_.close()

    # host-visible figures of the C boundary (wall time of the call, host sequences in, host hit lists out; never
    # `value`, which is quoted with the batch resident in HBM):
    #   stream     ONE bigsi_hip_search_stream call over several of the step's batches (the library pipelines its own chunks)
    #   one_call   bigsi_hip_search_batch latency for the step's first batch (if it is a batch of reads) and for a single query
    host_visible = {"two_workspace_loop_kmer_lookups_per_s": pcie_rate}
    if world == 1 and not args.force_dist and args.host_visible and args.full:
        lib_ = _lib.lib()
        # (the library's profiling events -- on since the timed region -- cost a stream 5-7 us per record: the latency figures
        # below are those of a library nobody is profiling, as scripts/call_breakdown.py measures them)
        check(lib_.bigsi_hip_set_profiling(st.handle, 0))
        want = 256 if w["batch"] * w["qlen"] < (1 << 17) else (8 if w["batch"] * w["qlen"] < (1 << 20) else 2)
        if w["score"]:
            want = max(want, 24)              # (six device batches of the library's own size: its pipeline in steady state)
        many = [s_ for i in range(want) for s_ in all_seqs[i % nb]]
        blob, soff = _lib.pack_seqs(many)
        n_many = len(many)
        hnk, hnu, hoff = np.zeros(n_many, np.uint32), np.zeros(n_many, np.uint32), np.zeros(n_many + 1, np.uint64)
        hcap = max(int(off[-1]) * want * 2, 1 << 16)
        hcol, hcnt = np.zeros(hcap, np.uint32), np.zeros(hcap, np.uint32)

        def stream_call():
            t_ = time.perf_counter()
            check(lib_.bigsi_hip_search_stream(st.handle, blob, _lib.ptr(soff), n_many, args.k, float(thr), 0, _lib.ptr(hnk), _lib.ptr(hnu), None,
                                               _lib.ptr(hoff), _lib.ptr(hcol), _lib.ptr(hcnt), hcap))
            return time.perf_counter() - t_
        stream_call()
        times = sorted(stream_call() for _ in range(5))
        assert np.array_equal(hnu[: w["batch"]], nu) and int(hoff[w["batch"]]) == int(off[-1])      # the first batch again, same answers
        host_visible["stream"] = {"kmer_lookups_per_s": float(hnu.sum()) / times[len(times) // 2], "best": float(hnu.sum()) / times[0],
                                  "sequences": n_many, "sequence_bytes": len(blob), "hits": int(hoff[-1]), "call_ms": times[len(times) // 2] * 1e3,
                                  "entry": "bigsi_hip_search_stream (one call; median of 5)"}

        from bigsi_amd.graph import bigsi as _front
        if args.dense and not w["score"] and _front._results is not None:
            # the reference's result dicts for the stream's hits (what BIGSI.search_stream yields), assembled from its arrays
            # (consumed as BIGSI.search_stream's caller consumes them: a sequence's list is dropped before the next one is looked at)
            t_, n_d = time.perf_counter(), 0
            for r_ in _front.native_result_lists(hnk, hnu, hoff.astype(np.int64), hcol, hcnt, exact, names, None, total_cols):
                n_d += len(r_)
            dt_ = time.perf_counter() - t_
            assert n_d == int(hoff[-1])
            host_visible["dicts"] = {"dicts_per_s": int(hoff[-1]) / dt_, "after_the_call_dicts_per_s": int(hoff[-1]) / (dt_ + times[len(times) // 2])}
        if w["score"]:
            # score=True through the boundary alone: ONE bigsi_hip_search_stream_scored call (sequences in; hit lists, presence
            # bits and score records out; each device batch's K5 + K6 beside the next batch's row-AND)
            from bigsi_amd.scoring import HIT_SCORE_DTYPE
            need = np.zeros(1, np.uint64)
            n_hits_many = int(hoff[-1])
            hboff, hrec = np.zeros(n_hits_many + 1, np.uint64), np.zeros(max(n_hits_many, 1), HIT_SCORE_DTYPE)
            words = (hnk.astype(np.int64) + 63) // 64
            hbits = np.zeros(max(int((words * np.diff(hoff).astype(np.int64)).sum()) * 8, 8), np.uint8)

            def scored_call():
                t_ = time.perf_counter()
                check(lib_.bigsi_hip_search_stream_scored(st.handle, blob, _lib.ptr(soff), n_many, args.k, float(thr), 0, _lib.ptr(hnk), _lib.ptr(hnu),
                                                          None, _lib.ptr(hoff), _lib.ptr(hcol), _lib.ptr(hcnt), n_hits_many, _lib.ptr(hbits), hbits.size,
                                                          _lib.ptr(hboff), _lib.ptr(hrec), _lib.ptr(need)))
                return time.perf_counter() - t_
            scored_call()
            times = sorted(scored_call() for _ in range(5))
            assert int(need[0]) == hbits.size and int(hoff[-1]) == n_hits_many and (hrec["num_kmers"][:n_hits_many] > 0).all()
            host_visible["stream_scored"] = {"kmer_lookups_per_s": float(hnu.sum()) / times[len(times) // 2], "best": float(hnu.sum()) / times[0],
                                             "hits": n_hits_many, "hits_per_s": n_hits_many / times[len(times) // 2],
                                             "bit_bytes": int(need[0]), "call_ms": times[len(times) // 2] * 1e3,
                                             "entry": "bigsi_hip_search_stream_scored (one call; median of 5)"}
            if _front._results is not None:
                # ... and as the reference's scored result dicts (22 keys + the presence string per hit), from the call's arrays
                t_, n_d = time.perf_counter(), 0
                for r_ in _front.native_result_lists(hnk, hnu, hoff.astype(np.int64), hcol, hcnt, exact, names, (hrec, hbits, hboff), total_cols):
                    n_d += len(r_)
                dt_ = time.perf_counter() - t_
                assert n_d == n_hits_many
                host_visible["scored_dicts"] = {"dicts_per_s": n_hits_many / dt_, "after_the_call_dicts_per_s": n_hits_many / (dt_ + times[len(times) // 2])}

        def one_call(seq_list, reps):
            bl, so = _lib.pack_seqs(seq_list)
            n_ = len(seq_list)
            a_, b_, c_ = np.zeros(n_, np.uint32), np.zeros(n_, np.uint32), np.zeros(n_ + 1, np.uint64)
            ts = []
            # (argument conversion hoisted out of the timed call: numpy's .ctypes.data alone is ~1 us per pointer, a quarter of a one-read call)
            argv = (st.handle, bl, _lib.ptr(so), n_, args.k, float(thr), 0, _lib.ptr(a_), _lib.ptr(b_), None, _lib.ptr(c_), _lib.ptr(hcol), _lib.ptr(hcnt), hcap)
            fn_ = lib_.bigsi_hip_search_batch
            for _ in range(reps + 3):
                t_ = time.perf_counter()
                rc_ = fn_(*argv)
                ts.append(time.perf_counter() - t_)
                check(rc_)
            return float(np.median(ts[3:]) * 1e6)
        host_visible["one_call_us"] = {"single_query": one_call(seqs[1:2], 100), "entry": "bigsi_hip_search_batch (the C call, median of 100)"}
        if w["batch"] * w["qlen"] < (1 << 17):
            host_visible["one_call_us"]["whole_batch_of_%d" % w["batch"]] = one_call(seqs, 100)

    # HBM traffic of this kernel on this workload, when a PMC pass for it has been committed (PMC counters cannot be
    # collected from inside the timed run; see profiles/)
    traffic, traffic_src = None, None
    wkey = "rows=%d cols=%d hashes=%d batch=%d qlen=%d k=%d threshold=%s draws=%d%s" % (
        w["rows"], my_cols, w["hashes"], w["batch"], w["qlen"], args.k, repr(float(thr)), args.and_draws, (" dense=1" if args.dense else "") + (" ee=1" if args.early_exit else ""))
    k5_ratio, k5_line_ratio, traffic_ratio_pmc = None, None, None
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
            ent = json.load(f).get(wkey) if args.full else None      # (roofline figures: --full)
        if ent:
            # the PMC pass measured launches of ITS shape (--timed resident: whole batches); what carries over to this run's launches --
            # a streamed thresholded batch goes out in two -- is the RATIO of traffic to algorithmic bytes (scaled below, once those are known)
            traffic, traffic_src = ent["traffic_bytes_per_launch"], ent["source"]
            traffic_ratio_pmc = ent.get("ratio")
            k5 = (ent.get("other_kernels") or {}).get("k_presence_bits")
            if k5 and ent.get("presence_alg_bytes_per_call"):
                # K5's HBM traffic over the algorithmic bytes of the whole K5 + K6 call (unique k-mers x h x 8 per distinct hit word + bits + records)
                k5_ratio = k5["traffic_bytes_per_launch"] / ent["presence_alg_bytes_per_call"]
                if ent.get("presence_line_floor_bytes_per_call"):      # ... and over the bytes of the 128-byte lines those words lie in (the hardware's floor)
                    k5_line_ratio = k5["traffic_bytes_per_launch"] / ent["presence_line_floor_bytes_per_call"]
    except OSError:
        pass

    verified = None
    if args.full and not args.no_verify:
        # EVERY rank: planted round trip on every shard (the gathered lists are identical on all ranks) + sampled queries against the
        # oracle on the rank's OWN shard (colours, counts; score=True: whole result dicts); rank 0 reports what all ranks found
        from oracle.ref_model import SynthOracle
        problem = None
        try:
            spans_cols = [my_cols] * world if args.scaling == "weak" else [n for _, n in plan_shards(w["cols"], parts)[1][:world]]
            for j, qi in enumerate(planted):
                hits = set(colours[int(off[qi]):int(off[qi + 1])].tolist())
                for g in range(world):
                    assert g * shard_cols + plant_col(j, g, spans_cols[g]) in hits, "planted query %d missing on shard %d" % (qi, g)
            orc = SynthOracle(SEED, rank, w["rows"], my_cols, w["hashes"], args.k, args.and_draws)
            for j, qi in enumerate(planted):
                orc.insert_kmers(plant_col(j, rank, my_cols), seqs[qi][:plant_len])
            sample = sorted(set([planted[0], 1 % w["batch"], w["batch"] // 2, w["batch"] - 1]))
            scored_sample = (0, min(15, w["batch"] - 1)) if w["score"] else ()
            if args.dense:
                # every plant of every staged batch counts (rows collide), but only the rows the checked queries read are kept
                only = np.unique(np.concatenate([orc.rows_of(seqs[qi]).ravel() for qi in set(sample) | set(scored_sample)]))
                if gene_dense:
                    for bi, qi, cols_d, segs_d in dense_gene_plants(w, nb, rank, my_cols, args.k):
                        orc.insert_kmer_masks(orc.rows_of(all_seqs[bi][qi]), cols_d, seg_masks(segs_d, n_kmers, args.k), only)
                else:
                    ones = np.ones((DENSE_READ_HITS, n_kmers), dtype=bool)
                    for bi in range(nb):
                        for r_, sq in enumerate(all_seqs[bi]):
                            orc.insert_kmer_masks(orc.rows_of(sq), dense_read_cols(bi, r_, rank, my_cols), ones, only)
            elif w["score"]:
                for bi, qi, c in score_plants(rank, my_cols):
                    orc.insert_kmers(c, all_seqs[bi][qi][:plant_len])
            for qi in sample:
                u, cnt = orc.counts(seqs[qi])
                want = np.flatnonzero(cnt >= (u if exact else mk[qi]))
                lo, hi = int(off[qi]), int(off[qi + 1])
                sel = (colours[lo:hi].astype(np.int64) // shard_cols) == rank          # this rank's shard
                assert u == nu[qi] and np.array_equal(colours[lo:hi][sel].astype(np.int64) - rank * shard_cols, want), "oracle mismatch on query %d" % qi
                assert np.array_equal(counts[lo:hi][sel], cnt[want].astype(np.uint32)), "oracle count mismatch on query %d" % qi
            n_scored = 0
            if w["score"]:
                # the result dicts of two planted queries of the first staged batch, whole lists, against the oracle's scorer
                from oracle import coracle
                from oracle.ref_model import Scorer as OracleScorer
                osc = OracleScorer(total_cols)
                for qi in scored_sample:
                    kmers, uniq, rows_q = orc.per_kmer_rows(seqs[qi])
                    cnt = coracle.unpack_and_sum(rows_q)[:my_cols]
                    u = len(uniq)
                    want_cols = [int(c) for c in np.flatnonzero(cnt >= (u if exact else int(np.ceil(u * thr))))]
                    if not exact:
                        want_cols.sort(key=lambda c: -int(cnt[c]))
                    qbits = np.unpackbits(rows_q, axis=1)
                    idx = {km: t for t, km in enumerate(uniq)}
                    got = scored["results"][qi]
                    assert [r["sample_name"] for r in got] == [names[c] for c in want_cols], "scored hit list of query %d differs from the oracle" % qi
                    for r, c in zip(got, want_cols):
                        col = "".join("1" if qbits[idx[km], c] else "0" for km in kmers)
                        want = {"percent_kmers_found": round(100 * float(cnt[c]) / u, 2), "num_kmers": u, "num_kmers_found": int(cnt[c]), "sample_name": names[c]}
                        want.update(osc.score(col))
                        want["kmer-presence"] = col
                        assert list(r) == list(want)
                        for key, v in want.items():
                            ok = abs(r[key] - v) <= 1e-12 * abs(v) + 2.5e-16 if key in ("evalue", "pvalue") else r[key] == v
                            assert ok, "score field %s of query %d sample %d: %r vs oracle %r" % (key, qi, c, r[key], v)
                        n_scored += 1
                assert n_scored >= 16
        except AssertionError as e:
            problem = "rank %d: %s" % (rank, e)
        found = [(problem, n_scored if problem is None else 0)]
        if use_dist:
            found = [None] * world
            dist.all_gather_object(found, (problem, n_scored if problem is None else 0))
        bad = [p_ for p_, _ in found if p_]
        if bad:
            raise SystemExit("bench.py: verification failed: " + "; ".join(bad))
        verified = "planted hits on %d shard(s) + %d queries == oracle (colours, counts) on EVERY shard" % (world, len(sample))
        if w["score"]:
            verified += "; %d scored dicts == oracle" % sum(n_ for _, n_ in found)

    line = None
    if rank == 0:
        ms_per_step = elapsed / args.steps * 1e3
        rate = total_unique / (elapsed / args.steps)
        resident = total_unique * resident_rate[0] / resident_rate[1] if resident_rate else None
        cr = sh.comm_ranks()
        whole = args.scaling == "strong" and parts == world
        line = {
            "metric": "kmer_lookups_per_s", "value": rate, "unit": "kmer_lookups/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None, "dtype": "u64", "data": "synthetic",
            "config": {
                "workload_short": "%s%s: %gM x %gk%s, h=%d, %d x %d bp/step, t=%g %s%s" % (
                    w["name"].replace("BASELINE ", ""), " (custom: %s)" % ",".join(args.custom) if args.custom else "", w["rows"] / 1e6,
                    (w["cols"] if args.scaling == "strong" else total_cols) / 1e3,
                    "" if whole and world == 1 else (" over %d GPUs" % world if whole else " (%d of %d shards)" % (world, parts) if args.scaling == "strong" else " weak"),
                    w["hashes"], w["batch"], w["qlen"], thr, "exact" if exact else "counts", ", score=True in the step" if w["score"] else ""),
                "exchange_ms": (warm.exchange_ms / warm.exchange_launches) if warm.exchange_launches else None,
                "calibration": cal,
                "workload": "%s%s: synthetic %d-row x %d-sample index%s, h=%d, %d x %d bp queries per step (%d staged batches), k=%d, "
                            "threshold=%g (%s)%s"
                            % (w["name"], " (shape overridden: %s)" % ",".join(args.custom) if args.custom else "", w["rows"],
                               w["cols"] if args.scaling == "strong" else total_cols,
                               "" if whole and world == 1 else
                               (" column-sharded over %d GPUs (%d samples each)" % (world, shard_cols) if whole else
                                " of which this run holds %d of %d column shards (%d samples)" % (world, parts, total_cols)
                                if args.scaling == "strong" else " = %d samples per GPU, weak scaling" % shard_cols),
                               w["hashes"], w["batch"], w["qlen"], nb, args.k, thr, "exact" if exact else "counts",
                               ", score=True: K5 + K6 + host assembly of every hit's scored result dict inside the step" if w["score"] else ""),
                "workload_key": args.workload, "rows": w["rows"], "cols_per_gpu": shard_cols, "total_cols": total_cols,
                "index_gb_per_gpu": info.index_bytes / 1e9, "hashes": w["hashes"], "batch": w["batch"], "qlen": w["qlen"],
                "unique_kmers_per_batch": total_unique, "hits_first_batch": int(off[-1]),
                "dense": None if not args.dense else
                ("first %d queries of every batch held, 0-%d SNPs apart, by %g %% of the shard's samples" % (DENSE_QUERIES, DENSE_MAX_SNPS, 100 * DENSE_COL_FRACTION)
                 if gene_dense else "every read held by %d samples" % DENSE_READ_HITS),
                "dense_plant_s": dense_s if args.dense else None,
                "early_exit": bool(args.early_exit) or None,
                "hits_per_s": int(off[-1]) / (elapsed / args.steps) if args.dense else None,
                "k5_traffic_ratio": k5_ratio, "k5_line_ratio": k5_line_ratio,
                "value_is": "unique query k-mers per second against the %d samples held by this run, exchange included; a step %s" % (
                    total_cols, "starts from sequences in HOST memory and ends with hit lists in host memory (SURVEY 8d (1)): %s" % (
                        "one bigsi_hip_search_stream call" if stream_steps else "batch reload (H2D) + sharded run + fetch of the gathered hit lists")
                    if host_steps else "runs a batch staged in HBM beforehand and leaves its hit lists on the device"),
                "value_inputs": "host" if host_steps else "resident", "resident_lookups_per_s": resident,
                "shard_lookups_per_s_sum": rate * world,
                "aggregate_GBps": sum(per_rank_gbs) if per_rank_gbs else None, "per_rank_GBps": per_rank_gbs or None,
                "parallelism": "column-shard x%d%s" % (world, "" if not use_dist else
                                                      " + ncclAllGather of 1 bit/sample (library-owned RCCL communicator)"
                                                      if sh.exchange == "rccl" else " + torch.distributed(%s) all-gather" % args.backend),
                "backend": args.backend if use_dist else None, "exchange": sh.exchange if use_dist else None,
                "rccl_ranks": cr[1] if cr else None, "ranks": ranks_info,
                "index_fill_s": fill_s, "index_contiguous": bool(stats.index_contiguous), "verified": verified, "presence": presence,
                "pcie_inclusive_kmer_lookups_per_s": pcie_rate,
                "host_visible": host_visible,
                "clocks": {"before_timed_region": clocks_before, "after_timed_region": clocks_after} if args.full else None,
            },
            "roofline": None if not args.full else {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                         "traffic": traffic_ratio_pmc * alg_bytes_launch if traffic_ratio_pmc else traffic, "traffic_source": traffic_src, "traffic_measured_in_run": False, "pmc_key": wkey,
                         "kernel": "k_reads_fused (K1 + row-AND + K4 in one launch)" if batch.info().one_launch else "k_and_exact" if exact else "k_and_count",
                         "alg_bytes_per_launch": alg_bytes_launch, "kernel_ms": and_ms, "launches_timed": int(stats.and_launches),
                         "kernel_ms_is": "alone on the device: one-stream pass of %d launches after the timed region (events); in the timed region launches overlap"
                                         % args.alone_steps if alone_ms else "HIP events around the kernel in the timed region",
                         "kernel_ms_overlapped": overlapped_ms, "frac_overlapped": alg_bytes_launch / (overlapped_ms * 1e-3) / 1e9 / HBM_PEAK_GBS if overlapped_ms else None,
                         "frac_of_box": achieved / cal[cal["compared_with"] + "_GBps"] if cal else None,
                         "launches_per_step": launches_per_step, "alg_bytes_per_step": alg_bytes,
                         # bytes of a step over the step's wall time: what the HBM delivers to the whole pipeline.  For batches of
                         # reads the one-launch kernels of consecutive steps overlap on the library's three read streams (one
                         # step's k-merising and compaction under its neighbours' row fetches), so each kernel's own duration
                         # -- `kernel_ms`, what `achieved` is priced on -- spans its neighbours too and exceeds the step time.
                         "step_GBps": alg_bytes / (ms_per_step * 1e-3) / 1e9, "step_frac": alg_bytes / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS,
                         "concurrent_launches": 3 if batch.info().one_launch and not args.one_stream else 1, "read_launches_repeated": repeated,
                         "rank": 0,
                         # per step, from warmup steps 2..W: K1 (+ row sort on the exact path); K4
                         "kmerize_ms": warm.kmerize_ms / (warmup - 1) if warmup > 1 else None,
                         "compact_ms": warm.compact_ms / (warmup - 1) if warmup > 1 else None},
        }
        if args.full and args.cpu_seconds > 0 and world == 1:        # reported at N=1 only
            line["cpu_baseline"] = cpu_baseline(args, w, my_cols, exact)
    for b_ in batches:
        b_.close()
    sh.close()
    st.delete_all()
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
        if legs is not None and rank == 0:
            shutil.rmtree(_sync_dir(), ignore_errors=True)      # (every rank is past the legs' last file barrier)
    if legs is None and want_legs(args):
        # one GPU: the other BASELINE configurations, each a short run of this script in a fresh process now that the index is freed
        legs = run_also_legs(args, world, rank)
    if rank == 0 and legs is not None:
        line["config"]["also"] = legs
    if rank == 0:
        if args.details:
            os.makedirs(os.path.dirname(os.path.abspath(args.details)) or ".", exist_ok=True)
            with open(args.details, "w") as f:
                json.dump(line, f, indent=1)
        # RCCL prints a version banner through C stdio (block-buffered when stdout is a pipe/file): flush it out first so
        # that the JSON line is the last thing on stdout
        import ctypes
        ctypes.CDLL(None).fflush(None)
        sys.stdout.flush()
        print(json.dumps(condense(line)), flush=True)


if __name__ == "__main__":
    main()
