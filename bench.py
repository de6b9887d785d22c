#!/usr/bin/env python3
"""Benchmark for the MI355X-native VictoriaLogs block-scan engine.

Headline workload (BASELINE.json configs[2] — the config the metric is
quoted on): 100M vlogsgenerator-shaped rows with 256-byte _msg,
AND(phrase on _msg, re2 regex on var_0) — the per-block filter evaluation
of lib/logstorage (blockSearch.search, block_search.go:207-226) rebuilt as
HIP kernels.  configs[1] (phrase-only) runs via --workload phrase.

A "step" is one pass of the hot path over the staged dataset: the filter
program is evaluated over every block's rows in ONE kernel launch, with
inputs already resident in HBM.  value = whole-job matched rows/sec across
all ranks (the headline filters match every generated row by construction,
so matched == scanned there; both fields are reported, and the all-match
invariant is asserted on every run).

A plain run does only what the headline figure needs: open the cached
fixture, stage it, warm up, time the steps, print the result line.  --full
adds the legs that take runs of their own: the full-size selectivity
self-check (a selective phrase whose expected count was recorded by the data
generator — gen_manifest.json, computed with plain string find, independent
of every scan path — must match exactly) and the CPU-oracle baseline.

The fixture is cached under --data-dir (default build/bench_data in this
tree); `bench.py --prepare-data` generates it without touching a GPU, and
build() does so on GPU hosts, so a benchmark run does not pay for it.

--dump-outputs DIR writes what the last timed step computed as float .npy
files (see dump_outputs()) so two builds can be compared output for output.

Usage: python bench.py [--gpus N] [--steps K] [--warmup W] [--rows R]
                       [--full] [--dump-outputs DIR]
For N>1 the driver launches this under torch.distributed.run, one rank per
GPU; the only collective is an all_reduce(SUM) of matched-row counters
(RCCL over xGMI).
"""

import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# fixture cache: inside the tree's (git-ignored) build directory, so it sits
# next to the libraries build() produced and `make clean` removes it
DEFAULT_DATA_DIR = os.path.join(ROOT, "build", "bench_data")

# --dump-outputs budget: the bitmaps are the only large array
DUMP_MAX_BITMAP_VALUES = 15_000_000  # float32 => 60 MB of the 64 MB allowed

HBM_PEAK_BYTES_PER_S = 8.0e12  # MI355X spec peak (MI355X_MICROARCH.md)

PHRASE_FILTER = '{"type":"phrase","field":"_msg","phrase":"message for the stream"}'
AND_REGEX_FILTER = (
    '{"type":"and","filters":['
    '{"type":"phrase","field":"_msg","phrase":"message for the stream"},'
    '{"type":"regexp","field":"var_0","re":"some value"}]}'
)
# selective phrase: matches rows whose random ip has first octet 77 (~1/256);
# the generator records the exact count per part in gen_manifest.json
SELECTIVE_FILTER = '{"type":"phrase","field":"_msg","phrase":"ip=77."}'

WORKLOADS = {
    # names match BASELINE.json configs[1]/[2] verbatim at the default 100M
    "phrase": {
        "name": "{rows} rows, phrase filter on _msg column, 1xMI355X "
                "(bloom + substring kernel)",
        "filter": PHRASE_FILTER,
        "expect_all": True,
    },
    "phrase_regex": {
        "name": "{rows} rows, AND(phrase, re2 regex) on two string columns, "
                "1xMI355X",
        "filter": AND_REGEX_FILTER,
        "expect_all": True,
    },
    "phrase_selective": {
        "name": "{rows} rows, selective phrase (ip=77., ~1/256 of rows) on "
                "_msg column",
        "filter": SELECTIVE_FILTER,
        "expect_manifest": "sel_msg_ip77",
    },
    # configs[3] shape (the driver shards it over N GPUs weak-scaling)
    "or8": {
        "name": "{rows} rows, OR of 8 phrase filters over 4 columns",
        "filter": '{"type":"or","filters":['
                  '{"type":"phrase","field":"_msg","phrase":"worker 3"},'
                  '{"type":"phrase","field":"_msg","phrase":"worker 5"},'
                  '{"type":"phrase","field":"dict_0","phrase":"error"},'
                  '{"type":"phrase","field":"dict_0","phrase":"fatal"},'
                  '{"type":"phrase","field":"dict_1","phrase":"warn"},'
                  '{"type":"phrase","field":"dict_1","phrase":"debug"},'
                  '{"type":"phrase","field":"host","phrase":"host_0"},'
                  '{"type":"phrase","field":"host","phrase":"host_9"}]}',
        # host_0 is a const column matching every generated row, so the OR
        # must match all rows — a full-size invariant like the headline's
        "expect_all": True,
    },
    "dict_time": {
        "name": "dict column + timestamp range (configs[4] shape)",
        "filter": '{"type":"and","filters":['
                  '{"type":"phrase","field":"dict_0","phrase":"error"},'
                  '{"type":"time","min":1700000000000000000,'
                  '"max":1700006250000000000}]}',
    },
}


def log(msg):
    print(f"[bench] {msg}", file=sys.stderr, flush=True)


def bench_nparts(rows, world):
    """Number of parts one rank's shard is split into."""
    return max(1, min(64, (os.cpu_count() or 8) // max(1, world),
                      max(8, rows // 16_000_000)))


def prepare_parts(data_dir, total_rows, nparts, msg_len, seed_base):
    """Generates nparts reference-format parts in parallel (cached on disk;
    gen_manifest.json is written last and doubles as a completion marker)."""
    from victorialogs_amd import generate_part

    os.makedirs(data_dir, exist_ok=True)
    dirs = []
    jobs = []
    rows_per = total_rows // nparts
    for i in range(nparts):
        rows = rows_per + (total_rows % nparts if i == nparts - 1 else 0)
        d = os.path.join(data_dir, f"part_{rows}_{msg_len}_{seed_base + i}")
        dirs.append(d)
        if not os.path.exists(os.path.join(d, "gen_manifest.json")):
            jobs.append((d, rows, seed_base + i))
    if jobs:
        t0 = time.time()
        log(f"generating {len(jobs)} parts ({total_rows} rows total)...")
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 8)) as ex:
            futs = [
                ex.submit(generate_part, d, rows, 1, 8192, msg_len, seed)
                for d, rows, seed in jobs
            ]
            for f in futs:
                f.result()
        log(f"generation took {time.time() - t0:.1f}s")
    return dirs


def stream_stages(data_dir, total_rows, nparts, msg_len, seed_base, filt,
                  device):
    """Generate -> stage -> delete, one part at a time (a window of parts is
    generated ahead on worker threads).  The GPU box's disk (~80 GB) cannot
    hold a 1B-row fixture (~65 GB of zstd parts plus headroom), but its HBM
    can hold the staged columns (~260 GB) — so parts stream through the disk
    while the staged arena accumulates.  One kernel launch per part-stage.
    Returns (stages, manifest_totals, rows, gen_stage_s, dims)."""
    import shutil
    from concurrent.futures import ThreadPoolExecutor

    from victorialogs_amd import Part, Stage, generate_part

    os.makedirs(data_dir, exist_ok=True)
    rows_per = total_rows // nparts
    specs = []
    for i in range(nparts):
        rows = rows_per + (total_rows % nparts if i == nparts - 1 else 0)
        d = os.path.join(data_dir, f"part_{rows}_{msg_len}_{seed_base + i}")
        specs.append((d, rows, seed_base + i))

    ahead = min(16, nparts)
    t0 = time.time()
    stages = []
    dims = []
    manifests = {}
    total = 0
    with ThreadPoolExecutor(max_workers=ahead) as ex:
        futs = {}

        def ensure(j):
            if j < len(specs) and j not in futs:
                d, rows, seed = specs[j]
                if os.path.exists(os.path.join(d, "gen_manifest.json")):
                    futs[j] = None
                else:
                    futs[j] = ex.submit(generate_part, d, rows, 1, 8192,
                                        msg_len, seed)

        for j in range(ahead):
            ensure(j)
        for i, (d, rows, seed) in enumerate(specs):
            if futs.get(i) is not None:
                futs[i].result()
            ensure(i + ahead)
            m = read_manifests([d])
            if m is not None:
                for k, v in m.items():
                    manifests[k] = manifests.get(k, 0) + v
            p = Part(d)
            st = Stage(p, filt, device=device)
            dims.append(part_dims(p))
            p.close()  # staging holds everything in HBM; files can go
            stages.append(st)
            total += st.rows
            shutil.rmtree(d, ignore_errors=True)
            if i % 8 == 0:
                log(f"streamed part {i + 1}/{len(specs)} "
                    f"({total} rows staged)")
    return stages, manifests, total, time.time() - t0, dims


def remove_partial_parts(rank_dir):
    """gen_manifest.json is written last; its absence marks a partial part
    stranded by a failed generation."""
    import glob
    import shutil
    for d in glob.glob(os.path.join(rank_dir, "part_*")):
        if not os.path.exists(os.path.join(d, "gen_manifest.json")):
            shutil.rmtree(d, ignore_errors=True)


def prepare_data(args):
    """--prepare-data: generates the single-GPU fixture a plain run would
    otherwise generate first, and nothing else (no GPU, no torch)."""
    rank_dir = os.path.join(args.data_dir, "rank0")
    try:
        prepare_parts(rank_dir, args.rows, bench_nparts(args.rows, 1),
                      args.msg_len, seed_base=1)
    except RuntimeError as e:
        if "short write" not in str(e):
            raise
        # the benchmark streams parts through a disk this small
        log(f"disk too small to cache the fixture ({e}); not cached")
        remove_partial_parts(rank_dir)


def part_dims(part):
    """(blocks, bitmap words) of a part: one bitmap per block, padded to
    whole 64-bit words (the layout vql_fetch_bitmaps returns)."""
    nblocks = part.blocks
    return nblocks, sum((part.block_rows(i) + 63) // 64
                        for i in range(nblocks))


def dump_outputs(out_dir, stages, dims, last_hits, suffix=""):
    """Writes what a caller of the timed path holds after its last step:

    hits.npy       float64[stages]  matched rows each scan() returned
    block_hits.npy float64[blocks]  per-block matched rows
    bitmaps.npy    float32[words*4] the result bitmaps, 16 bits per value
                   (little-endian: value k of word w holds rows 64w+16k ..
                   64w+16k+15 of the block), so every value is exact

    Past DUMP_MAX_BITMAP_VALUES the bitmaps are reduced to a fixed seeded
    sample of their 16-bit values (same positions on every run)."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    block_hits = []
    chunks = []
    for st, (nblocks, nwords) in zip(stages, dims):
        block_hits.extend(st.fetch_block_hits(nblocks))
        chunks.append(np.frombuffer(st.fetch_bitmaps(nwords), dtype="<u2"))
    bits = np.concatenate(chunks) if chunks else np.zeros(0, dtype="<u2")
    if bits.size > DUMP_MAX_BITMAP_VALUES:
        idx = np.unique(np.random.default_rng(0).integers(
            0, bits.size, DUMP_MAX_BITMAP_VALUES))
        bits = bits[idx]
    np.save(os.path.join(out_dir, f"hits{suffix}.npy"),
            np.asarray(last_hits, dtype=np.float64))
    np.save(os.path.join(out_dir, f"block_hits{suffix}.npy"),
            np.asarray(block_hits, dtype=np.float64))
    np.save(os.path.join(out_dir, f"bitmaps{suffix}.npy"),
            bits.astype(np.float32))


def read_manifests(part_dirs):
    """Sums the generator-recorded selective counts over this rank's parts."""
    totals = {}
    for d in part_dirs:
        p = os.path.join(d, "gen_manifest.json")
        if not os.path.exists(p):
            return None
        with open(p) as f:
            m = json.load(f)
        for k, v in m.items():
            totals[k] = totals.get(k, 0) + v
    return totals


def load_pmc_traffic(workload):
    """PMC-counter HBM traffic per launch for this workload, from the
    committed rocprofv3 collection (separate --pmc passes; gfx950 FETCH_SIZE
    correction applied per MI355X_MICROARCH.md).  None if not collected."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                        "profiles", "r02", "pmc_traffic.json")
    try:
        with open(path) as f:
            data = json.load(f)
        ent = data.get(workload)
        if not ent:
            return None, None
        traffic = ent.get("fetch_bytes_per_launch", 0) + ent.get(
            "write_bytes_per_launch", 0)
        return traffic, ent.get("source")
    except (OSError, ValueError):
        return None, None


def cpu_baseline(part_dirs, filter_json, budget_s=20.0):
    """Times the CPU oracle (restatement of the reference's Go scan path —
    no Go toolchain exists on this image) on a bounded sample
    of the same workload, all host cores."""
    from victorialogs_amd import OracleScanner

    threads = os.cpu_count() or 8
    orc = OracleScanner(part_dirs[0])
    try:
        nblocks = orc.blocks
        # calibrate on a few blocks
        t0 = time.perf_counter()
        probe_blocks = min(8, nblocks)
        orc.scan(filter_json, lo=0, hi=probe_blocks, threads=threads)
        dt = max(time.perf_counter() - t0, 1e-6)
        per_block = dt / probe_blocks
        sample_blocks = min(nblocks, max(probe_blocks, int(budget_s / per_block)))
        rows = sum(orc.block_rows(i) for i in range(sample_blocks))
        # repeat the sample until >=2s of measured work (a single-part scan
        # at 256 threads finishes in ~0.1s and was too noisy)
        reps = 0
        t0 = time.perf_counter()
        dt = 0.0
        while dt < min(2.0, budget_s) or reps < 1:
            orc.scan(filter_json, lo=0, hi=sample_blocks, threads=threads)
            reps += 1
            dt = time.perf_counter() - t0
        return {
            "value": rows * reps / dt,
            "unit": "rows/s",
            "cores": threads,
            "kind": "port",
            "sample": f"{sample_blocks} blocks / {rows} rows of the same part "
                      f"x {reps} passes, {dt:.1f}s on {threads} host threads "
                      f"(C++ oracle restatement; reference Go binary not "
                      f"buildable here)",
        }
    finally:
        orc.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rows", type=int,
                    default=int(os.environ.get("VQL_BENCH_ROWS", 100_000_000)))
    ap.add_argument("--msg-len", type=int, default=256)
    ap.add_argument("--workload", choices=sorted(WORKLOADS),
                    default="phrase_regex")
    ap.add_argument("--data-dir", default=os.environ.get(
        "VQL_DATA_DIR", DEFAULT_DATA_DIR))
    ap.add_argument("--full", action="store_true",
                    help="also run the legs that take runs of their own: "
                         "the full-size selectivity self-check and the CPU "
                         "oracle baseline")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last step "
                         "computed as DIR/<name>.npy")
    ap.add_argument("--prepare-data", action="store_true",
                    help="generate the cached single-GPU fixture for "
                         "--rows/--msg-len and exit (needs no GPU)")
    ap.add_argument("--skip-cpu-baseline", action="store_true",
                    help="with --full: leave the CPU baseline out")
    ap.add_argument("--skip-selectivity", action="store_true",
                    help="with --full: leave the selectivity check out")
    ap.add_argument("--stream-parts", action="store_true",
                    help="generate->stage->delete parts one at a time so "
                         "configs whose fixture exceeds the box disk (1B "
                         "rows) still stage fully into HBM; implies "
                         "--skip-cpu-baseline/--skip-selectivity (the part "
                         "files are gone after staging)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.prepare_data:
        prepare_data(args)
        return
    if not args.full:
        args.skip_cpu_baseline = True
        args.skip_selectivity = True

    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    distributed = world > 1
    ndev = torch.cuda.device_count() if torch.cuda.is_available() else 0
    device = local_rank % ndev if ndev else 0
    # RCCL over xGMI when each rank owns a GPU (the driver's 8-GPU run);
    # RCCL refuses two ranks on one device ("Duplicate GPU detected"), so a
    # world-2 test on a 1-GPU box runs the SAME distributed branches with
    # gloo carrying the three tiny counter all_reduces while the scans still
    # run on the GPU; gloo also lets the world-2 CPU CI test run (emu build)
    backend = "nccl" if ndev and world <= ndev else "gloo"
    coll_dev = "cuda" if backend == "nccl" else "cpu"
    if distributed:
        dist.init_process_group(backend)
        if ndev:
            torch.cuda.set_device(device)

    from victorialogs_amd import Filter, Part, Stage

    wl = WORKLOADS[args.workload]
    filter_json = wl["filter"]

    # Each rank generates and stages its own shard (weak scaling; blocks are
    # independent units, storage_search.go:1035-1067).
    nparts = bench_nparts(args.rows, world)
    filt = Filter(filter_json)
    dims = []  # per-stage (blocks, bitmap words), for --dump-outputs
    if args.stream_parts:
        args.skip_cpu_baseline = True
        args.skip_selectivity = True
        part_dirs = []
        parts = []
        stages, manifest, _, stage_s, dims = stream_stages(
            os.path.join(args.data_dir, f"rank{rank}"), args.rows, nparts,
            args.msg_len, 1000 * rank + 1, filt, device)
    else:
        try:
            part_dirs = prepare_parts(
                os.path.join(args.data_dir, f"rank{rank}"), args.rows, nparts,
                args.msg_len, seed_base=1000 * rank + 1)
            manifest = read_manifests(part_dirs)

            log(f"rank {rank}: staging {len(part_dirs)} parts onto device "
                f"{device}")
            t0 = time.time()
            parts = [Part(d) for d in part_dirs]
            # one multi-part stage: the whole pass is ONE kernel launch
            stages = [Stage(parts, filt, device=device)]
            stage_s = time.time() - t0
        except RuntimeError as e:
            if "short write" not in str(e):
                raise
            # disk too small for the full fixture (e.g. 8 ranks sharing an
            # ~80 GB box disk): stream parts through the disk instead
            log(f"rank {rank}: disk full ({e}); falling back to "
                "--stream-parts")
            remove_partial_parts(os.path.join(args.data_dir, f"rank{rank}"))
            args.skip_cpu_baseline = True
            args.skip_selectivity = True
            part_dirs = []
            parts = []
            stages, manifest, _, stage_s, dims = stream_stages(
                os.path.join(args.data_dir, f"rank{rank}"), args.rows, nparts,
                args.msg_len, 1000 * rank + 1, filt, device)
    staged_bytes = sum(s.staged_bytes for s in stages)
    algo_bytes = sum(s.algo_bytes for s in stages)
    rows = sum(s.rows for s in stages)
    live_rows = sum(s.live_rows for s in stages)
    log(f"rank {rank}: staged {staged_bytes / 1e9:.2f} GB "
        f"({rows} rows, {live_rows} live) in {stage_s:.1f}s")

    last_hits = [0] * len(stages)  # what each stage's latest scan() returned

    def one_step():
        kms = 0.0
        for i, s in enumerate(stages):
            last_hits[i] = s.scan()
            kms += s.last_kernel_ms
        return sum(last_hits), kms

    # warmup + full-size correctness property (all-match invariant): the
    # headline filters match every generated row by construction, so the
    # device count must equal the staged row count
    hits = 0
    for _ in range(max(args.warmup, 1)):
        hits, _ = one_step()
    if wl.get("expect_all") and hits != rows:
        raise SystemExit(
            f"correctness check failed: {args.workload} workload matched "
            f"{hits} of {rows} rows (expected all)")
    exp_key = wl.get("expect_manifest")
    if exp_key is not None:
        if manifest is None:
            raise SystemExit("no gen_manifest.json for selective workload")
        if hits != manifest[exp_key]:
            raise SystemExit(
                f"correctness check failed: {args.workload} matched {hits}, "
                f"generator recorded {manifest[exp_key]}")

    # timed region: barrier + sync on both sides, MAX over ranks
    if distributed:
        dist.barrier()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    kernel_ms_total = 0.0
    for _ in range(args.steps):
        hits, kms = one_step()
        kernel_ms_total += kms
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    if distributed:
        dist.barrier()
    elapsed = time.perf_counter() - t0

    if args.dump_outputs:
        if parts:
            # one multi-part stage holding every block of every part
            per_part = [part_dims(p) for p in parts]
            dims = [(sum(b for b, _ in per_part), sum(w for _, w in per_part))]
        dump_outputs(args.dump_outputs, stages, dims, last_hits,
                     suffix=f"_rank{rank}" if distributed else "")

    # whole-job aggregation: MAX(elapsed) over ranks; SUM(rows, hits)
    if distributed:
        dev = coll_dev
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        c = torch.tensor([float(rows), float(hits), float(algo_bytes)],
                         dtype=torch.float64, device=dev)
        dist.all_reduce(c, op=dist.ReduceOp.SUM)
        total_rows, total_hits, total_algo = (int(c[0].item()), int(c[1].item()),
                                              int(c[2].item()))
    else:
        total_rows, total_hits, total_algo = rows, hits, algo_bytes

    ms_per_step = elapsed * 1000.0 / args.steps
    rows_per_s = total_rows * args.steps / elapsed
    gb_per_s = total_algo * args.steps / elapsed / 1e9
    matched_per_s = total_hits * args.steps / elapsed

    # roofline for the dominant (only) kernel, HIP-event timed per launch on
    # its own stream; algorithmic bytes per launch / avg launch duration.
    avg_kernel_s = (kernel_ms_total / 1000.0) / (args.steps * max(1, len(stages)))
    algo_per_launch = algo_bytes / max(1, len(stages))
    achieved = algo_per_launch / avg_kernel_s if avg_kernel_s > 0 else 0.0
    traffic, traffic_src = load_pmc_traffic(args.workload)
    roofline = {
        "bound": "hbm",
        "achieved": achieved,
        "peak": HBM_PEAK_BYTES_PER_S,
        "unit": "B/s",
        "frac": achieved / HBM_PEAK_BYTES_PER_S,
        # PMC-counter HBM bytes per launch from the committed rocprofv3
        # collection on this workload's single-launch kernel (separate --pmc
        # passes cannot run inside the timed region)
        "traffic": traffic,
        "traffic_source": traffic_src,
        "kernel": "scan_program_kernel",
        "avg_kernel_ms": avg_kernel_s * 1000.0,
    }

    # full-size selectivity self-check: a filter with a
    # generator-known expected count != rows must match it exactly — a
    # kernel writing all-ones bitmaps fails here
    sel = None
    run_sel = (not args.skip_selectivity and manifest is not None
               and args.workload in ("phrase", "phrase_regex"))
    if distributed:
        # ranks must agree (a rank that fell back to stream-parts has no
        # files left to restage and skips; mismatched schedules would hang
        # the all_reduce below)
        t = torch.tensor([0.0 if run_sel else 1.0], dtype=torch.float64,
                         device=coll_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        run_sel = t.item() == 0.0
    if run_sel:
        log("selectivity self-check (phrase ip=77.)...")
        sfilt = Filter(SELECTIVE_FILTER)
        sstage = Stage(parts, sfilt, device=device)
        got = sstage.scan()
        t0 = time.perf_counter()
        sel_steps = 3
        for _ in range(sel_steps):
            got = sstage.scan()
        sel_elapsed = time.perf_counter() - t0
        expected = manifest["sel_msg_ip77"]
        sstage.close()
        sfilt.close()
        if distributed:
            dev = coll_dev
            c = torch.tensor([float(expected), float(got)],
                             dtype=torch.float64, device=dev)
            dist.all_reduce(c, op=dist.ReduceOp.SUM)
            expected, got = int(c[0].item()), int(c[1].item())
        if got != expected:
            raise SystemExit(
                f"selectivity check FAILED: matched {got}, generator "
                f"recorded {expected}")
        sel = {
            "filter": SELECTIVE_FILTER,
            "expected_matches": expected,
            "got_matches": got,
            "ok": True,
        }
        if world == 1:
            sel["scanned_rows_per_sec"] = rows * sel_steps / sel_elapsed

    result = None
    if rank == 0:
        cb = None
        if world == 1 and not args.skip_cpu_baseline:
            log("timing CPU baseline (oracle restatement)...")
            cb = cpu_baseline(part_dirs, filter_json)
        result = {
            "metric": "matched-rows/sec",
            "value": matched_per_s,
            "unit": "rows/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u8",
            "data": "synthetic",
            "config": {
                "workload": wl["name"].format(
                    rows=f"{args.rows // 10**6}M" if args.rows >= 10**6
                    else str(args.rows)),
                "rows_per_gpu": rows,
                "live_rows_per_gpu": live_rows,
                "msg_len": args.msg_len,
                "filter": filter_json,
                "matched_rows_per_pass": total_hits,
                "parallelism": f"dp{world}",
            },
            # matched == scanned for the all-match headline filters; they
            # diverge on selective workloads (report both)
            "scanned_rows_per_sec": rows_per_s,
            "matched_rows_per_sec": matched_per_s,
            "gb_scanned_per_sec": gb_per_s,
            "hbm_resident_bytes": staged_bytes * world,
            "roofline": roofline,
            # end-to-end (cold) path: host zstd decode + H2D staging + one
            # scan (§8d "clearly separated"; the reference re-decompresses
            # values blocks per scan, block_search.go:444-474)
            "cold": {
                "stage_s": stage_s,
                "staged_gb": staged_bytes / 1e9,
                "rows_per_s_incl_staging": rows / (stage_s + ms_per_step / 1e3),
            },
            "selectivity_check": sel,
            "cpu_baseline": cb,
        }
        print(json.dumps(result), flush=True)

    for s in stages:
        s.close()
    filt.close()
    for p in parts:
        p.close()
    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
