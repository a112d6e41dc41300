#!/usr/bin/env python3
"""bench.py -- IQ Msamples/s through demod+FEC at 48 kS/s per channel (BASELINE.json metric).

One "step" = one pass of the hot path (demodulator + framer/FEC) over one batch of synthetic RS41 IQ that is
already resident in HBM.  N=1 workload = BASELINE.json configs[1]: 1024 synthetic RS41-SG channels on one MI355X.
With N>1 every rank owns its own shard of channels (channels are independent: no data-path collective, weak
scaling).  `python bench.py --gpus N` works as typed: without a torchrun environment it re-executes itself
under torch.distributed.run with N ranks on 127.0.0.1.

Prints ONE JSON line on rank 0 (DESIGN.md section 6 has the roofline accounting).
This file is the contract: arguments, the headline workload, roofline / traffic / cpu_baseline, the line.  Everything else it measures
-- the other BASELINE configurations riding in the same line, --mix (configs[2]), --wideband (configs[3]), the multi-GPU runs -- lives
in bench_configs.py.

A plain run (`bench.py --gpus 1 --steps K --warmup W`) does only what the headline needs: it builds the resident blocks, ramps the clock,
warms up, times exactly K steps, writes the last step's outputs if --dump-outputs is given and prints the line (metric, value, unit,
ms_per_step, ...).  Everything else -- kernel-timing events, the HBM read probe, the rocprofv3 trace / counter sub-runs (roofline,
traffic), frame counts, the CPU baseline, the other configurations, the back-to-back layout and the low-SNR point -- runs with --full.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

# the CPU baseline's OpenMP threads must sleep, not spin, between parallel regions: a spinning 256-thread
# team starves the single-thread measurement that follows it (has to be set before any OpenMP runtime loads)
os.environ.setdefault("OMP_WAIT_POLICY", "passive")
os.environ.setdefault("GOMP_SPINCOUNT", "0")

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import bench_configs
from bench_configs import (CLASS_NAMES, HBM_PEAK_GBS, JOIN_NAMES, alg_bytes_of, make_blocks, measure, restride, run_node, run_wideband,
                           scattered_blocks, small_run)


def effective_cpus() -> int:
    """CPUs this process may actually use: the scheduler affinity mask, cut down by a cgroup CPU quota if there is one
    (os.cpu_count() is the machine's, not the container's)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]) + 0.5)))
            else:
                q = int(txt[0])
                if q > 0:
                    per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                    n = min(n, max(1, int(q / per + 0.5)))
            break
        except (OSError, ValueError, IndexError):
            continue
    return max(1, n)


def free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--ramp-ms", type=float, default=250.0,
                    help="untimed submits for this long before the warmup steps: the GPU idles at 157 MHz and needs ~0.1 s of load "
                         "to reach its 2.35 GHz working clock; a 3-step warmup (1 ms) measures the ramp, not the kernel")
    ap.add_argument("--channels", type=int, default=None, help="channels per GPU (default: 1024, BASELINE configs[1]; with --mix 4096, configs[2])")
    ap.add_argument("--blocks", type=int, default=5, help="headline workload: consecutive blocks of a continuous, seamlessly repeating signal "
                    "held in HBM and cycled through (1: the same block every step; 5 x 96 tiles = 32 frame periods)")
    ap.add_argument("--tiles", type=int, default=96, help="2048-sample tiles per channel per step (96 = 4.096 s)")
    ap.add_argument("--ebn0", type=float, default=14.0)
    ap.add_argument("--cpu-channels", type=int, default=0, help="channels of the CPU baseline sample (0 = auto)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="wall time spent on the all-thread CPU baseline sample")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--mix", action="store_true", help="BASELINE configs[2]: sonde type = (RS41, M10, DFM09)[channel %% 3] (not the headline workload)")
    ap.add_argument("--sonde-type", type=int, default=0, help="all channels of this SONDE_* type (1 DFM09, 2 iMS-100, 3 M10; not the headline workload)")
    ap.add_argument("--wideband", action="store_true", help="BASELINE configs[3]: 10 MS/s IQ -> 512-bin channelizer -> per-bin demod+FEC")
    ap.add_argument("--wb-streams", type=int, default=1, help="--wideband: independent 10 MS/s streams processed per step")
    ap.add_argument("--wb-dual", action="store_true", help="--wideband: both stackings of every stream (even + odd-stacked bank: 1024 channels per stream, "
                    "every carrier within 4.9 kHz of a bin centre)")
    ap.add_argument("--wb-iq16", action="store_true", help="--wideband: the blocks as int16 I, Q pairs (sonde_chan_set_input: what a 10 MS/s receiver delivers)")
    ap.add_argument("--wb-overlap", action="store_true", help="--wideband: filter bank and decoder on two internal streams (consecutive submits may overlap)")
    ap.add_argument("--wb-blocks", type=int, default=1, choices=(1, 2, 4, 8), help="--wideband: blocks of 1 280 000 samples (0.128 s) per submit")
    ap.add_argument("--wb-occupied", type=int, default=16, help="--wideband: bins of every stream that carry an RS41 transmitter (16: a sparse band; 256: every other bin, the FEC stage busy)")
    ap.add_argument("--time-every", type=int, default=None, help="kernel-timing HIP events on every n-th timed step (1: all; with --full default 8, "
                    "4 for runs of fewer than 16 steps; a plain run records none).  A timed step carries two event records of 6.4 us of command-stream bubble each "
                    "(profiles/r2_notes.md), inside the timed region: every 8th costs 0.6 %% of the step")
    ap.add_argument("--flags", type=int, default=None, help="SondeBatchConfig.flags (1: wide, 2: FEC as its own kernel, 4: never-joined launch units, 32: launch units joined "
                    "one submit late; default 0 = ordinary stream semantics)")
    ap.add_argument("--time-slices", type=int, default=0, help="experiment: SondeBatchConfig.time_slices (0: the library's choice, 1: never, n: n segments per channel and submit)")
    ap.add_argument("--iq16", action="store_true", help="experiment: ONLY the 16-bit integer IQ entry at --channels x --tiles (prints its record)")
    ap.add_argument("--iq8", action="store_true", help="experiment: ONLY the 8-bit integer IQ entry at --channels x --tiles (prints its record)")
    ap.add_argument("--no-others", action="store_true", help="headline only: skip the other BASELINE configurations (other_configs), the low-SNR "
                    "line and the rocprofv3 traffic passes that the default run appends")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)     # the sub-run rocprofv3 --pmc wraps (roofline.traffic)
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)   # the sub-run rocprofv3 --kernel-trace wraps (roofline.kernel_us_trace)
    ap.add_argument("--stride-pad", type=int, default=0, help="experiment: extra samples between channels in HBM (overrides --row-stride)")
    ap.add_argument("--row-stride", choices=("pow2", "contiguous"), default="pow2",
                    help="layout of the resident IQ blocks: rows on the library's recommended channel stride (sonde_row_stride: the next power of "
                         "two in bytes, 2 MiB for the headline's 1.5 MiB rows; measured 2.3-5.5 %% faster, profiles/r3_stride_sweep.txt) or back to back")
    ap.add_argument("--scatter", action="store_true", help="(the default with --gpus > 1) ingest on rank 0 and scatter IQ shards over RCCL before timing")
    ap.add_argument("--scatter-torch", action="store_true", help="(kept for old command lines: --multiproc always scatters through torch.distributed now)")
    ap.add_argument("--multiproc", action="store_true", help="--gpus > 1: one process per GPU (torch.distributed ranks, torch.distributed.scatter of the ingest blocks) instead of the default: ONE "
                    "process driving every GPU through the native node-level host (sonde_node_*, ncclCommInitAll)")
    ap.add_argument("--node", action="store_true", help="run through the node-level host even with --gpus 1 (a node of one device: test hook)")
    ap.add_argument("--rank-local", action="store_true", help="--gpus > 1: every rank generates its own shard (no scatter): kernel scaling without xGMI time")
    ap.add_argument("--full", action="store_true", help="besides the headline: kernel-timing events (default --time-every), the HBM read probe, roofline "
                    "and traffic (rocprofv3 sub-runs), frame counts, the CPU baseline, the other BASELINE configurations, the back-to-back layout "
                    "and the low-SNR point (--no-cpu / --no-others trim it); without it the line carries the headline figures only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write the frames the last timed step produced "
                    "(what sonde_batch_frames hands a caller, ordered by channel and bit position) as DIR/frames_<field>.npy, at most 64 MB")
    args = ap.parse_args()
    if args.trace_child:      # the headline workload itself, 60 timed steps, no timing events: nothing printed
        args.steps, args.warmup, args.ramp_ms, args.no_cpu, args.no_others, args.time_every = 60, 20, 150.0, True, True, 0
        args.full, args.dump_outputs = True, None
    elif args.pmc_child:      # a short headline-shaped run for the counter passes: one block re-submitted, nothing printed
        args.steps, args.warmup, args.ramp_ms, args.blocks, args.no_cpu, args.no_others, args.time_every = 10, 2, 60.0, 1, True, True, 0
        args.full, args.dump_outputs = True, None
    return args


# the fields of a SondeFrame record (sdrpp_radiosonde_amd._lib.FRAME_DTYPE), each dumped as one array
DUMP_FIELDS = ("channel", "type", "len", "nerr", "flags", "bitpos", "data")
DUMP_MAX_BYTES = 60_000_000          # (the .npy headers come on top: the whole dump stays under 64 MB)


def dump_frames(dirname, frames, prefix=""):
    """The frames of one submit as DIR/<prefix>frames_<field>.npy: `data` (the frame bytes) in float32, the other fields in float64
    (integers below 2**53: exact).  At most DUMP_MAX_BYTES in all: a larger submit is cut to a fixed, seeded sample of its frames
    (the headline's ~4 000 frames per step take ~9 MB and are written whole).  Returns the number of frames written."""
    per_frame = frames.dtype["data"].shape[0] * 4 + sum(int(np.prod(frames.dtype[f].shape or (1,))) * 8 for f in DUMP_FIELDS if f != "data")
    keep = DUMP_MAX_BYTES // per_frame
    if len(frames) > keep:
        frames = frames[np.sort(np.random.default_rng(12345).choice(len(frames), keep, replace=False))]
    os.makedirs(dirname, exist_ok=True)
    for f in DUMP_FIELDS:
        np.save(os.path.join(dirname, f"{prefix}frames_{f}.npy"), frames[f].astype(np.float32 if f == "data" else np.float64))
    return len(frames)


def cpu_baseline(iq, C, n, args):
    """The oracle (plain-C restatement, OpenMP over channels) on this host's cores, on a bounded sample of the same
    channels.  Single thread first (>= 1 s of work, nothing else running), then a sweep over thread counts on a short
    sample, then whole passes with the best count until --cpu-seconds of wall time are spent."""
    import oracle_lib
    cores = effective_cpus()
    cc = args.cpu_channels or C
    host_iq = iq[:cc].contiguous().cpu().numpy()           # (the resident block may be a view of a padded allocation)
    # ---- one thread: channels one at a time until >= 1.2 s have been spent
    oracle_lib.batch_run(0, host_iq[:1, :2048 * 4], nthreads=1)            # load the library, touch the code
    t1, c1 = 0.0, 0
    while t1 < 1.2 and c1 < cc:
        t0 = time.perf_counter()
        oracle_lib.batch_run(0, host_iq[c1:c1 + 1], nthreads=1)
        t1 += time.perf_counter() - t0
        c1 += 1
    single = c1 * n / t1 / 1e6
    # ---- thread-count sweep on a short sample (about 1 s each at the single-thread rate x threads)
    cands = sorted({t for t in (1, 2, 4, 8, 16, 32, 64, 128, cores) if t <= cores})
    sweep = {}
    for t in cands:
        if t == 1:
            sweep[1] = round(single, 3)
            continue
        k = int(min(cc, max(t, min(4 * t, t * single * 1e6 / n))))     # >= one channel per thread, about 1 s
        t0 = time.perf_counter()
        oracle_lib.batch_run(0, host_iq[:k], nthreads=t)
        sweep[t] = round(k * n / (time.perf_counter() - t0) / 1e6, 3)
    best_t = max(sweep, key=lambda t: sweep[t])
    # ---- the reported figure: whole passes over the sample with the best thread count
    passes, cdt, nref = 0, 0.0, 0
    while cdt < args.cpu_seconds:
        t0 = time.perf_counter()
        ref = oracle_lib.batch_run(0, host_iq, nthreads=best_t)
        cdt += time.perf_counter() - t0
        passes += 1
        nref = int(len(ref))
    # ---- the conventional per-sample receiver (oracle/or_yardstick.c: channel filter, libm atan2f, AGC, per-symbol Gardner loop;
    # the yardstick of tests/test_yardstick.py) on a smaller sample of the same channels: what a textbook CPU decoder costs
    conv = None
    try:
        ck = int(min(cc, max(best_t, 4 * best_t)))
        t0 = time.perf_counter()
        nconv = int(len(oracle_lib.yard_run(0, host_iq[:ck], nthreads=best_t)))
        ct = time.perf_counter() - t0
        conv = {"value": round(ck * n / ct / 1e6, 3), "unit": "Msamples/s", "cores": best_t, "kind": "conventional",
                "sample": f"one pass over {ck} of the same channels x {n} samples ({ct:.1f} s wall), oracle/or_yardstick.c", "frames": nconv}
    except Exception as e:      # the baseline proper does not depend on it
        conv = {"error": f"{type(e).__name__}: {e}"}
    return {"value": round(passes * cc * n / cdt / 1e6, 3), "unit": "Msamples/s", "cores": best_t, "kind": "port", "conventional": conv,
            "sample": f"{passes} passes over {cc} of the same channels x {n} samples ({cdt:.1f} s wall), oracle/ (plain C, "
                      f"OpenMP over channels); thread count = best of the sweep",
            "host_cpus": {"affinity": len(os.sched_getaffinity(0)), "effective": cores, "os_cpu_count": os.cpu_count()},
            "thread_sweep_msps": {str(k): v for k, v in sweep.items()},
            "single_thread_msps": round(single, 3),
            "single_thread_sample": f"{c1} channels x {n} samples, {t1:.2f} s, before any multi-thread run",
            "frames_per_pass": nref}


def main():
    args = parse_args()
    # ---- N > 1 (or --node): ONE process drives every GPU through the product's C++ node-level host (include/sonde_node.h:
    # ncclCommInitAll, scatter of IQ rows over xGMI, one decoder batch per GPU) -- north_star's "C++ host code ... sharded across the 8
    # GPUs of one node with an RCCL scatter" (VERDICT r4 item 2).  Under the driver's torchrun launch (one rank per GPU) rank 0 is that
    # process and the other ranks wait at a host-side barrier; `--multiproc` keeps round 4's one-process-per-GPU path.
    node_mode = (args.gpus > 1 or args.node) and not args.multiproc and not args.wideband and not args.mix and not args.sonde_type \
        and os.environ.get("SONDE_BENCH_BACKEND", "nccl") != "gloo"
    if node_mode and torch.cuda.is_available() and torch.cuda.device_count() >= args.gpus:
        if args.dump_outputs:
            sys.exit("bench.py: --dump-outputs covers the one-process-per-GPU channel path (not the node host: add --multiproc)")
        world = int(os.environ.get("WORLD_SIZE", "1"))
        rank = int(os.environ.get("RANK", "0"))
        dist = None
        if world > 1:                              # the driver's launch: the ranks only rendezvous (gloo: no device work on ranks > 0)
            import torch.distributed as dist
            import datetime
            dist.init_process_group("gloo", timeout=datetime.timedelta(minutes=60))
        if rank == 0:
            out = run_node(args, launched_ranks=world)
            print(json.dumps(out), flush=True)
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N --multiproc` as typed: spawn the ranks ourselves (one process per GPU, rendezvous on 127.0.0.1)
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU (there is no CPU fallback)")
    # SONDE_BENCH_BACKEND=gloo is a test hook: it lets the N>1 code path run on a box with fewer GPUs than
    # ranks (ranks share devices, scalars are reduced on the host).  The driver's runs use RCCL ("nccl").
    backend = os.environ.get("SONDE_BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    if backend == "gloo":
        local_rank %= ndev
    elif ndev < world:
        sys.exit(f"bench.py: --gpus {world} needs {world} visible GPUs, this node has {ndev} (SONDE_BENCH_BACKEND=gloo shares devices for tests)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    nccl_ranks = None
    if world > 1:
        import torch.distributed as dist
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
        # which device every rank sits on, as the collective backend sees it (all-gather of device identities)
        props = torch.cuda.get_device_properties(local_rank)
        ident = f"{socket.gethostname()}:{local_rank}:{getattr(props, 'uuid', props.name)}"
        objs = [None] * world
        dist.all_gather_object(objs, ident)
        nccl_ranks = {"backend": "rccl" if backend == "nccl" else backend, "world": world, "distinct_devices": len(set(objs))}
        if backend == "nccl" and nccl_ranks["distinct_devices"] != world:
            sys.exit(f"bench.py: {world} ranks sit on {nccl_ranks['distinct_devices']} distinct devices: one process per GPU is the contract")
    red_dev = dev if backend == "nccl" else torch.device("cpu")

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def reduce_max_sum(dt, count):
        if dist is None:
            return dt, float(count)
        t = torch.tensor([dt], device=red_dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        c = torch.tensor([count], device=red_dev, dtype=torch.float64)
        dist.all_reduce(c, op=dist.ReduceOp.SUM)
        return float(t.item()), float(c.item())

    if args.dump_outputs and (args.wideband or args.iq16 or args.iq8):
        sys.exit("bench.py: --dump-outputs covers the channel path (not --wideband, --iq16, --iq8)")
    if args.wideband:
        out = run_wideband(args, rank, local_rank, world, dev, barrier, reduce_max_sum)
    else:
        out = run_channels(args, rank, local_rank, world, dev, dist, barrier, reduce_max_sum)
    if out is None:                                  # --pmc-child: the run rocprofv3 wraps; nothing to print
        return
    if nccl_ranks is not None:
        out["nccl_ranks"] = nccl_ranks
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


def measured_traffic(args):
    """HBM bytes per launch of the demod kernel from rocprofv3 PMC counters, measured NOW: two separate --pmc passes
    (FETCH_SIZE takes 3 of the 4 TCC slots, WRITE_SIZE 2: MI355X_MICROARCH.md) over a 10-step sub-run of this script with the
    headline shape; FETCH_SIZE is doubled (gfx950 tallies the 128-byte requests of wide coalesced reads at 64 B, same guide).
    Returns (bytes, source text) or (None, reason)."""
    import shutil
    import sqlite3
    import tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None, "rocprofv3 not found"
    if any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ):
        return None, "this process is itself being profiled (rocprofv3 environment present): no nested counter passes"
    C = args.channels or 1024
    vals = {}
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="sonde_pmc_", dir="/tmp")
        cmd = [exe, "--pmc", ctr, "-d", d, "-o", "pmc", "--", sys.executable, os.path.abspath(__file__), "--pmc-child",
               "--channels", str(C), "--tiles", str(args.tiles), "--ebn0", str(args.ebn0), "--blocks", "1"]
        env = dict(os.environ, TMPDIR="/tmp")
        try:
            r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=240)
            dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(d) for f in fs if f.endswith(".db")]
            if r.returncode != 0 or not dbs:
                return None, f"rocprofv3 --pmc {ctr} failed (rc {r.returncode}): {(r.stderr or r.stdout)[-200:]}"
            db = sqlite3.connect(dbs[0])
            # the counter is reported per dispatch (summed over its instances): average over the sub-run's launches
            rows = db.execute("select dispatch_id, sum(value) from counters_collection where kernel_name like '%sd_demod_kernel%' "
                              "and counter_name = ? group by dispatch_id", (ctr,)).fetchall()
            if not rows:
                return None, f"no {ctr} samples for sd_demod_kernel in the rocprofv3 output"
            vals[ctr] = sum(v for _, v in rows) / len(rows)
        except (subprocess.TimeoutExpired, sqlite3.Error, OSError) as e:
            return None, f"rocprofv3 --pmc {ctr}: {e}"
        finally:
            shutil.rmtree(d, ignore_errors=True)
    fetch = vals["FETCH_SIZE"] * 1024 * 2          # KiB; x2: gfx950 correction for wide coalesced reads
    write = vals["WRITE_SIZE"] * 1024
    return int(fetch + write), ("measured in this run: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE (separate passes) over a 10-step "
                                f"sub-run of this command's shape ({C} channels x {args.tiles} tiles); FETCH_SIZE x2 (gfx950 correction) = "
                                f"{int(fetch)} B + WRITE_SIZE {int(write)} B per launch")


def traced_kernel_us(args):
    """Average duration (us) of the demod kernel from a rocprofv3 --kernel-trace pass over a sub-run of this script with the
    headline shape and workload (five blocks cycled, 60 timed steps, no timing events in the stream): the figure
    `rocprofv3 --kernel-trace --stats` prints for the same command, measured NOW.  The first launches of the sub-run (clock
    ramp, warmup) are dropped.  Returns (us, launches averaged, note) or (None, 0, reason)."""
    import shutil
    import sqlite3
    import tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None, 0, "rocprofv3 not found"
    if any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ):
        return None, 0, "this process is itself being profiled: no nested trace pass"
    C = args.channels or 1024
    d = tempfile.mkdtemp(prefix="sonde_trace_", dir="/tmp")
    cmd = [exe, "--kernel-trace", "-d", d, "-o", "trace", "--", sys.executable, os.path.abspath(__file__), "--pmc-child", "--trace-child",
           "--channels", str(C), "--tiles", str(args.tiles), "--ebn0", str(args.ebn0), "--blocks", str(args.blocks),
           "--row-stride", getattr(args, "row_stride", "pow2")]
    try:
        r = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True, timeout=300)
        dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(d) for f in fs if f.endswith(".db")]
        if r.returncode != 0 or not dbs:
            return None, 0, f"rocprofv3 --kernel-trace failed (rc {r.returncode}): {(r.stderr or r.stdout)[-200:]}"
        rows = sqlite3.connect(dbs[0]).execute("select start, end from kernels where name like '%sd_demod_kernel%' order by start").fetchall()
        rows = rows[-60:]                          # the timed steps of the sub-run (ramp and warmup launches come first)
        if len(rows) < 20:
            return None, 0, "too few sd_demod_kernel launches in the trace"
        us = sum(e - b for b, e in rows) / len(rows) / 1e3
        return us, len(rows), (f"rocprofv3 --kernel-trace over a SEPARATE sub-run of this command's shape (profiler attached, its own clocks: "
                               f"may read a fraction of a percent above or below this run's ms_per_step), last {len(rows)} launches")
    except (subprocess.TimeoutExpired, sqlite3.Error, OSError) as e:
        return None, 0, f"rocprofv3 --kernel-trace: {e}"
    finally:
        shutil.rmtree(d, ignore_errors=True)


def headline_config(args, kind, C, n, world, blocks, m, scatter):
    return {"workload": (f"RS41/M10/DFM09 by channel % 3 x {C} channels/GPU x {n} samples (48 kS/s)" if kind == "mix" else
                         f"SONDE type {args.sonde_type} x {C} channels/GPU x {n} samples (48 kS/s)" if args.sonde_type else
                         f"RS41-SG x {C} channels/GPU x {n} samples per step (4800 Bd GFSK, 48 kS/s, Eb/N0 {args.ebn0} dB)")
                        + (f"; {len(blocks)} consecutive blocks of a continuous signal resident in HBM, cycled" if len(blocks) > 1 else ""),
            "channels_per_gpu": C, "samples_per_channel": n, "sharding": f"channels/{world}", "flags": args.flags,
            "launch_units": m["launch"]["units"], "join": JOIN_NAMES[m["launch"]["join"]] if m["launch"]["units"] > 1 else "one launch on the caller's stream",
            "channel_stride_samples": int(blocks[0].stride(0) // 2),
            "layout": ("rows back to back" if int(blocks[0].stride(0) // 2) == n else
                       f"rows {int(blocks[0].stride(0) // 2) * 8 // 1024} KiB apart (sonde_row_stride; --row-stride contiguous puts them back to back)"),
            "ingest": "rank-local" if scatter is None else scatter["ingest"]}


def headline_line(args, kind, m, blocks, C, n, world, dt, scatter, dumped):
    """The figures of the K timed steps that every run prints (a plain run prints nothing else; --full adds to it)."""
    msps = C * n * world * args.steps / dt / 1e6
    out = {
        "metric": "IQ Msamples/s through demod+FEC @ 48 kS/s/ch",
        "value": round(msps, 3),
        "unit": "Msamples/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ramp_ms": args.ramp_ms,
        "ms_per_step": round(dt / args.steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": headline_config(args, kind, C, n, world, blocks, m, scatter),
        "realtime_channels": round(msps * 1e6 / 48000.0, 1),
        "full": bool(args.full),
    }
    if scatter is not None:
        out["scatter"] = scatter
        out["scatter_ms"] = scatter["ms"]
    if dumped:
        out["outputs_dumped"] = dict(dumped, dir=args.dump_outputs)
    return out


def run_channels(args, rank, local_rank, world, dev, dist, barrier, reduce_max_sum):
    from sdrpp_radiosonde_amd import _lib
    import ctypes

    if args.channels is None:
        args.channels = 4096 if args.mix else 1024
    if args.time_every is None:
        args.time_every = (8 if args.steps >= 16 else 4) if args.full else 0      # (a plain run records no timing events)
    if args.flags is None:
        args.flags = 0
    C, n = args.channels, args.tiles * 2048
    stream = torch.cuda.current_stream().cuda_stream
    kind = "mix" if args.mix else (args.sonde_type if args.sonde_type else "rs41")
    if args.iq16 or args.iq8:
        rec = small_run(kind, C, args.tiles, args.blocks, args.flags, args, local_rank, dev, barrier, stream, iq16=args.iq16, iq8=args.iq8, steps=args.steps, warmup=args.warmup)
        if rank == 0:
            print(json.dumps(rec))
        return None
    default_run = args.full and kind == "rs41" and world == 1 and not args.no_others and not args.pmc_child
    scatter = None
    if os.environ.get("SONDE_BENCH_BACKEND", "nccl") == "gloo":
        args.scatter_torch = True                  # test hook (ranks share devices): RCCL needs one device per rank
    if world > 1 and kind == "rs41" and not args.rank_local:
        blocks, types, scatter = scattered_blocks(args, rank, local_rank, world, dev, dist, barrier)
    else:
        blocks, types = make_blocks(kind, C, args.tiles, args.blocks, args.ebn0, dev, seed=1000 + rank, first_channel=rank * C)
    if not (scatter is not None and scatter.get("rows_delivered_strided")):      # (the native scatter delivers strided rows itself)
        blocks = restride(blocks, args)
    dumped = {}

    def dump(batch):                                 # the last timed step's frames, before anything else is submitted
        frames = batch.frames()
        dumped["frames"] = dump_frames(args.dump_outputs, frames, prefix=f"rank{rank}_" if world > 1 else "")
        dumped["of"] = int(len(frames))

    m = measure(blocks, types, args.flags, args, local_rank, barrier, stream, counts=args.full, after_timed=dump if args.dump_outputs else None,
                ramp_decoder=True)
    if args.pmc_child:
        return None
    dt, nfr_total = reduce_max_sum(m["dt"], m["nfr_step"] or 0)
    out = headline_line(args, kind, m, blocks, C, n, world, dt, scatter, dumped)
    if not args.full:
        return out
    demod_ms, framer_ms = m["demod_ms"], m["framer_ms"]

    # read-only streaming kernel over the same IQ buffer: what this GPU's HBM delivers to a pure read
    gbs = ctypes.c_float(0.0)
    if _lib.load().sonde_hbm_read_probe(ctypes.c_void_p(blocks[0].data_ptr()), C * n * 8, 10, ctypes.byref(gbs)) != 0:
        raise RuntimeError(_lib.last_error())
    achievable = float(gbs.value)

    ms_per_step = dt / args.steps * 1e3
    # roofline of the dominant kernel (the demodulator): algorithmic bytes = 8 B per complex64 sample read once
    # + bits written (n/sps/8 bytes per channel) -- DESIGN.md section 6
    alg_bytes = alg_bytes_of(C, n)
    pipelined = m["launch"]["units"] > 1 and m["launch"]["join"] != 0      # launch units that overlap from submit to submit
    if pipelined:
        demod_ms = ms_per_step        # the classes of consecutive submits overlap: there is no per-step kernel interval; see kernel_ms
    step_achieved = alg_bytes / (ms_per_step * 1e-3) / 1e9
    # the dominant kernel's duration: the rocprofv3 kernel trace of a sub-run (default run); else the library's HIP events, which
    # bracket the launch with two event records (a few us of command-stream bubble each) and therefore read HIGH: a kernel cannot
    # take longer than the step that contains it, so the event figure is capped at the step (VERDICT r3 weak point 6)
    trace_us, trace_n, trace_note = (None, 0, None)
    if default_run and rank == 0:
        trace_us, trace_n, trace_note = traced_kernel_us(args)
    events_ms = m["demod_ms"]
    if not pipelined and events_ms > 0:
        demod_ms = min(events_ms, ms_per_step)
    kernel_src = "HIP events around every %dth launch, capped at ms_per_step" % args.time_every if args.time_every else "none"
    if trace_us is not None and not pipelined:
        demod_ms = trace_us * 1e-3
        kernel_src = trace_note
    if demod_ms <= 0:
        demod_ms = ms_per_step
        kernel_src = "ms_per_step (no kernel timing in this run)"
    achieved = alg_bytes / (demod_ms * 1e-3) / 1e9
    # HBM traffic per launch: measured now by two rocprofv3 --pmc passes over a sub-run (default run); otherwise, and as the
    # labelled fallback, REPLAYED from the committed passes of the same command (profiles/*_traffic.json)
    traffic, traffic_source = None, None
    if default_run and rank == 0:
        traffic, traffic_source = measured_traffic(args)
    if traffic is None:
        why = traffic_source
        for name in ("r3_traffic.json", "r2_traffic.json", "r1_traffic.json"):
            try:
                tj = json.load(open(os.path.join(ROOT, "profiles", name)))
                if tj["channels_per_gpu"] == C and tj["samples_per_channel"] == n and kind == "rs41":
                    traffic = tj["fetch_bytes"] + tj["write_bytes"]
                    traffic_source = (f"replayed from profiles/{name} (separate rocprofv3 --pmc passes of this command on the builder's box, "
                                      "FETCH_SIZE x2 gfx950 correction); not measured in this run" + (f" ({why})" if why else ""))
                    break
            except (OSError, KeyError, ValueError):
                continue

    kernel_ms = {"demod": round(demod_ms, 4), "framer_fec": round(framer_ms, 4), "demod_hip_events_raw": round(events_ms, 4),
                 "note": f"demod = the figure roofline.frac uses ({kernel_src}); demod_hip_events_raw = HIP events on every {args.time_every}th timed "
                         "step, which include the event records' own command-stream bubbles; for RS41 the demod kernel includes sync search and FEC"}
    if m["class_ms"]:
        kernel_ms["per_class"] = {CLASS_NAMES[k]: round(v, 4) for k, v in m["class_ms"].items()}
        if pipelined:
            kernel_ms["note"] += ("; pipelined class streams: `demod` spans a submit's fork to its completion and overlaps the neighbouring "
                                  "submits, per_class = each class's demod kernel alone")
    out.update({
        "frames_per_s": round(nfr_total * args.steps / dt, 1),
        "frames_per_step_steady": round(nfr_total, 2),
        "frames_first_submit": m["nfr_first"],
        "kernel_ms": kernel_ms,
        "roofline": {"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBS, 4),
                     "step_achieved": round(step_achieved, 2), "step_frac": round(step_achieved / HBM_PEAK_GBS, 4),
                     "kernel_us_trace": None if trace_us is None else round(trace_us, 2), "kernel_us_trace_launches": trace_n,
                     "kernel_time_source": kernel_src,
                     "traffic": traffic, "traffic_source": traffic_source,
                     "achievable_read": round(achievable, 1), "frac_of_achievable": round(achieved / achievable, 4),
                     "algorithmic_bytes": alg_bytes, "kernel": "sd_demod_kernel (dominant kernel of the step; frac = algorithmic bytes / its duration [kernel_time_source], step_frac = the same bytes / the whole step by the wall clock)"},
    })
    if rank == 0 and world == 1 and not args.no_cpu and kind == "rs41":
        out["cpu_baseline"] = cpu_baseline(blocks[0], C, n, args)
        out["cpu_baseline"]["frames_match_gpu_first_submit"] = bool(out["cpu_baseline"]["frames_per_pass"] == m["nfr_first"]) \
            if (args.cpu_channels or C) == C else None
    if default_run:
        # ---- the other BASELINE configurations, the back-to-back layout and the low-SNR point, measured in this same process
        # (bench_configs.py: everything that is not the headline)
        del blocks
        torch.cuda.empty_cache()
        out.update(bench_configs.other_configs(args, rank, local_rank, world, dev, barrier, reduce_max_sum, stream, C))
    return out


if __name__ == "__main__":
    main()
