#!/usr/bin/env python3
"""bench.py — LZ4 encode+decode GiB/s (device-resident), 64 KiB blocks, 1/2/4/8 GPUs.

Workload (BASELINE.json configs[1]): 4096 x 64 KiB synthetic
log-text blocks per GPU, resident in HBM before the timed region. One step = one pass of
the hot path over the batch: encode every block into an LZ4 frame (lz4_flex layout:
FLG 0x64, BD 0x40, xxh32 content checksum; frames packed contiguously) then decode every
frame back (frame walk, block decode, xxh32 verify). value = uncompressed bytes of all
ranks / (max over ranks of the timed wall time), i.e. U / (t_enc + t_dec).

Multi-GPU: one process per GPU, blocks sharded across ranks with no
data-path collective; a gloo (CPU) group provides the barrier and the max-over-ranks
reduction of the timed interval. `--gpus N` works both ways:
  * under torch.distributed.run (WORLD_SIZE set): this process is one rank; WORLD_SIZE must
    equal N;
  * standalone: this process spawns N fresh rank processes (RANK/LOCAL_RANK/WORLD_SIZE,
    rendezvous on 127.0.0.1) before anything touches the GPU, waits for them and relays
    rank 0's line.
Default weak scaling: 4096 blocks per GPU (config 2 per GPU). `--total-blocks 1048576` is
config 5's strong-scaling split (131,072 blocks = 8 GiB per GPU at N = 8).

A plain run sets up, warms up, times the steps and prints the line: `value`, `ms_per_step` and
the two rooflines that the timed steps' own HIP events give (the match finder k_enc_parse, and
`roofline_decode`, the north_star's decode figure: C + U per launch of the whole decode over
its launch time). `--dump-outputs DIR` also writes what the last timed step computed as .npy
files. Everything else is behind `--full`: the output checks (the gate after the warm-up and
every decoded byte after the timed steps), `--profile-steps` extra steps with every phase timed
(`kernel_ms_per_step`, which kernel dominates, `roofline_decode_kernels`) and `cpu_baseline`,
which times the CPU port of the reference path (oracle/: the lz4_flex FrameEncoder/FrameDecoder
restatement) on every host core over a bounded sample of the same workload (rank 0, N = 1
only): median of 5 runs of >= 1 s.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(ROOT, "sample-s3-hybrid-cache_amd")]

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md: 8.0 TB/s spec, 6.3 measured)
METRIC = "LZ4 encode+decode GiB/s (device-resident), 64 KiB blocks, 1/2/4/8 GPU"
GiB = float(1 << 30)
CHUNK_BLOCKS = 4096  # synthetic input is generated / uploaded / checked 256 MiB at a time


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=4096, help="64 KiB blocks per GPU (config 2: 4096; weak scaling)")
    ap.add_argument("--total-blocks", type=int, default=0,
                    help="strong scaling instead: split this many blocks over the ranks (config 5: 1048576)")
    ap.add_argument("--full", action="store_true",
                    help="also check the outputs, time every phase in extra steps (kernel_ms_per_step, the dominant "
                         "kernel's roofline) and run the CPU baseline; a plain run only times the steps")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (see dump_outputs)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave the CPU baseline out")
    ap.add_argument("--pipeline", action="store_true",
                    help="two queues: step k's decode overlaps step k+1's encode (rooflines then include overlap)")
    ap.add_argument("--profile-steps", type=int, default=3,
                    help="with --full: extra steps after the timed region, every phase timed (kernel_ms_per_step)")
    ap.add_argument("--no-kernel-timing", action="store_true",
                    help="diagnostics: no HIP events in the timed steps (no roofline; measures the events' cost)")
    ap.add_argument("--skip-check", action="store_true", help="with --full, diagnostic builds only: skip output checks")
    ap.add_argument("--cpu-seconds", type=float, default=1.0, help="wall seconds of each of the 5 CPU baseline runs")
    ap.add_argument("--selftest", action="store_true",
                    help="launcher/rank plumbing only (no GPU): every rank reports in, rank 0 prints the summary")
    ap.add_argument("--share-gpu", action="store_true",
                    help="rehearsal only: allow more ranks than visible GPUs (ranks then share devices; "
                         "the line says so). Without it, N ranks on fewer than N devices are refused")
    return ap.parse_args(argv)


# ------------------------------------------------------------------ launcher (no GPU in here)
def _free_port() -> int:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(n: int, argv, timeout: float = 1800.0) -> int:
    """Run this script as n rank processes (fresh interpreters, never an exec of this one);
    relay rank 0's stdout. Returns the exit code (first failing rank's, else 0). All ranks are
    polled together: as soon as one exits non-zero (or the overall timeout passes) the others are
    killed, so a rank that dies before a collective cannot leave rank 0 blocked in gloo."""
    import threading
    import time

    port = _free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   GROUP_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    chunks = []
    reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    deadline = time.monotonic() + timeout
    rc = 0
    while True:
        codes = [p.poll() for p in procs]
        bad = [c for c in codes if c not in (None, 0)]
        if bad:
            rc = bad[0]
            break
        if all(c == 0 for c in codes):
            break
        if time.monotonic() > deadline:
            sys.stderr.write(f"bench.py: ranks still running after {timeout:g} s; killing them\n")
            rc = 124
            break
        time.sleep(0.05)
    for p in procs:
        if p.poll() is None:
            p.kill()
        p.wait()
    reader.join(timeout=10)
    sys.stdout.write(b"".join(c for c in chunks if c).decode())
    sys.stdout.flush()
    return rc


def launch_decision(args):
    """None = run as a rank in this process; int = exit code of the spawned ranks."""
    ws = os.environ.get("WORLD_SIZE")
    if ws is not None:
        if int(ws) != args.gpus:
            sys.stderr.write(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={ws}: refusing to mislabel the run\n")
            return 2
        return None
    if args.gpus > 1:
        return spawn_ranks(args.gpus, sys.argv[1:])
    return None


def selftest(args):
    import shard

    fail = os.environ.get("S3HC_SELFTEST_FAIL_RANK")  # launcher test: this rank dies before any collective
    if fail is not None and int(fail) == int(os.environ.get("RANK", "0")):
        sys.exit(3)
    g = shard.Group()
    total = args.total_blocks or args.blocks * g.world
    lo, hi = shard.shard_range(total, g.world, g.rank) if args.total_blocks else (g.rank * args.blocks, (g.rank + 1) * args.blocks)
    g.barrier()
    ranks = g.sum(1.0)
    blocks = g.sum(float(hi - lo))
    if g.rank == 0:
        print(json.dumps({"selftest": True, "n_gpus": g.world, "ranks_reporting": int(ranks),
                          "blocks_total": int(blocks), "scaling": "strong" if args.total_blocks else "weak"}))
    g.close()


# ------------------------------------------------------------------ CPU baseline (rank 0, N = 1)
def host_cpu_info():
    model = None
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    quota = None
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()
        quota = None if q == "max" else round(int(q) / int(p), 2)
    except (OSError, ValueError):
        pass
    return model, quota


def cpu_baseline(data_chunk: bytes, block: int, seconds: float):
    """Oracle (C port of the reference path) on every host core, encode+decode per block:
    median of 5 runs of >= `seconds` wall each, plus a single-thread run."""
    import ctypes
    import statistics

    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O  # CPU baseline leg only

    L = O.lib()
    L.or_bench_blocks.restype = ctypes.c_int
    L.or_bench_blocks.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_double,
                                  ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_double),
                                  ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    nb = len(data_chunk) // block
    buf = ctypes.create_string_buffer(data_chunk, len(data_chunk))

    def run(threads, secs, fixed=0):
        done, wall, es, ds = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        rc = L.or_bench_blocks(buf, nb, block, threads, secs, fixed, ctypes.byref(done), ctypes.byref(wall),
                               ctypes.byref(es), ctypes.byref(ds))
        assert rc == 0, f"cpu baseline round trip failed ({rc})"
        return done.value, wall.value, es.value, ds.value

    n1, w1, e1, d1 = run(1, seconds)
    affinity = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    model, quota = host_cpu_info()
    # effective cores: the CPUs this process may run on, capped by the cgroup CPU quota (a 16-CPU
    # quota on a 256-thread host runs 16 threads' worth of work whatever the thread count)
    threads = max(1, min(affinity, int(quota))) if quota else affinity
    runs = []
    for _ in range(5):
        n, w, _, _ = run(threads, seconds)
        runs.append(n * block / w / GiB)
    over = None
    if threads < affinity:  # the same run oversubscribed to every thread of the affinity mask
        n, w, _, _ = run(affinity, seconds)
        over = round(n * block / w / GiB, 4)
    # a labelled third-party C reference: liblz4's raw block API on the same
    # blocks and threads — not the proxy's codec (no frames, no content checksum, its own parser)
    lz4 = None
    L.or_bench_blocks_liblz4.restype = ctypes.c_int
    L.or_bench_blocks_liblz4.argtypes = L.or_bench_blocks.argtypes
    probe = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    if L.or_bench_blocks_liblz4(buf, nb, block, 1, 0.0, 1, *[ctypes.byref(x) for x in probe]) == 0:
        def run_lz4(th, secs):
            done, wall, es, ds = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
            rc = L.or_bench_blocks_liblz4(buf, nb, block, th, secs, 0, ctypes.byref(done), ctypes.byref(wall),
                                          ctypes.byref(es), ctypes.byref(ds))
            assert rc == 0, f"liblz4 baseline round trip failed ({rc})"
            return done.value, wall.value, es.value, ds.value
        ln1, lw1, le1, ld1 = run_lz4(1, seconds)
        lr = []
        for _ in range(3):
            n, w, _, _ = run_lz4(threads, seconds)
            lr.append(n * block / w / GiB)
        lz4 = {"value": round(statistics.median(lr), 4), "unit": "GiB/s", "cores": threads,
               "kind": "third-party C LZ4 (liblz4 1.9.3), not the proxy's codec",
               "sample": "LZ4_compress_default + LZ4_decompress_safe per 64 KiB block of the same batch (raw "
                         "blocks: no frame, no xxh32), same threads and ranges; median of 3 runs",
               "runs_gibps": [round(x, 4) for x in lr],
               "single_thread_gibps": round(ln1 * block / lw1 / GiB, 4),
               "single_thread_encode_gibps": round(ln1 * block / le1 / GiB, 4),
               "single_thread_decode_gibps": round(ln1 * block / ld1 / GiB, 4)}
    return {
        "value": round(statistics.median(runs), 4),
        "unit": "GiB/s",
        "cores": threads,
        "kind": "port",
        "sample": f"64 KiB blocks of the bench's own log-text batch ({nb} distinct blocks, cycled), lz4_flex-faithful "
                  f"frame encode + decompress_data per block (oracle/ C port, -O3), {threads} threads (effective "
                  f"cores = min(affinity {affinity}, cgroup quota {quota})) over contiguous block ranges; median of "
                  f"5 runs of >= {seconds:g} s wall",
        "runs_gibps": [round(x, 4) for x in runs],
        "oversubscribed_all_threads_gibps": over,
        "single_thread_gibps": round(n1 * block / w1 / GiB, 4),
        "single_thread_encode_gibps": round(n1 * block / e1 / GiB, 4),
        "single_thread_decode_gibps": round(n1 * block / d1 / GiB, 4),
        "host_nproc": os.cpu_count(),
        "cpu_affinity": affinity,
        "cgroup_cpu_quota": quota,
        "cpu_model": model,
        "third_party_liblz4": lz4,
    }


# ------------------------------------------------------------------ device assignment
def assign_device(world: int, local: int, ndev: int, share: bool):
    """(device index, None) for this rank, or (None, reason) when the run must be refused: N ranks
    on fewer than N visible devices would report N "GPUs" that are fewer GPUs (one process per
    GPU). --share-gpu makes it an explicit rehearsal instead."""
    if ndev <= 0:
        return None, "no visible GPU"
    if world > ndev and not share:
        return None, (f"{world} ranks but only {ndev} visible GPU(s): refusing to report {world} GPUs "
                      f"(pass --share-gpu for a shared-device rehearsal)")
    if local >= ndev and not share:
        return None, f"LOCAL_RANK {local} has no GPU of its own ({ndev} visible)"
    return local % ndev, None


# ------------------------------------------------------------------ the GPU bench (one rank)
# decode: the fast path's token index + executor (k_dtok + k_dexec; k_decode_pe then only exits for
# the units they took), or with S3HC_FAST=0 / S3HC_FAST_DISABLE the parser + executor kernel
# (k_decode_pe; S3HC_DEC_ONEWAVE=1 selects the one-wave kernel)
_FAST_OFF = bool(os.environ.get("S3HC_FAST_DISABLE")) or os.environ.get("S3HC_FAST", "") == "0"
KERNEL_SYMBOL = {"enc_parse": "k_enc_parse", "enc_emit": "k_enc_emit",
                 "decode": ("k_decode_units" if os.environ.get("S3HC_DEC_ONEWAVE") else "k_decode_pe") if _FAST_OFF
                 else "k_dtok+k_dexec+k_decode_pe",
                 "dec_close": "k_dframe_close"}


def pmc_traffic(kernel):
    """HBM bytes per launch of `kernel` from the newest committed rocprofv3 PMC summary
    (profiles/rNN/traffic.json, made by tools/traffic.sh from this same bench command:
    FETCH_SIZE and WRITE_SIZE in separate --pmc passes, per-dispatch averages in KB).
    FETCH_SIZE is doubled: on gfx950 it counts half the bytes of 16-B/lane streaming reads."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*", "traffic.json")))
    if not files:
        return None, None
    d = json.load(open(files[-1]))
    total = 0.0
    for part in KERNEL_SYMBOL.get(kernel, kernel).split("+"):  # a phase of several kernels: their sum
        k = d.get(part, {})
        if "FETCH_SIZE" not in k or "WRITE_SIZE" not in k:
            return None, None
        total += 2 * k["FETCH_SIZE"] + k["WRITE_SIZE"]
    return int(total * 1024), os.path.relpath(files[-1], ROOT)


def roofline_obj(kt, name, alg_bytes, profiled_shape: bool):
    ms, n = kt[name]
    per_launch_s = ms / n / 1e3
    achieved = alg_bytes / per_launch_s / 1e9
    # the committed PMC summary is of the default command (4096 blocks); other shapes get none
    traffic, tsrc = pmc_traffic(name) if profiled_shape else (None, None)
    roof = {
        "bound": "hbm", "kernel": KERNEL_SYMBOL.get(name, name), "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
        "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic,
        "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_ms": round(ms / n, 4),
    }
    if tsrc:
        roof["traffic_source"] = tsrc + " (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, same bench command)"
        roof["traffic_bound"] = TRAFFIC_BOUND
    return roof


# FETCH_SIZE is doubled for every kernel: the guide's halving applies to wide (16-B/lane) coalesced
# streaming reads; for narrow gathers (k_dexec's sources, k_enc_parse's staged-input reads are LDS)
# the doubled figure over-counts, so `traffic` is an upper bound of the HBM bytes
TRAFFIC_BOUND = "upper: FETCH_SIZE x2 for every kernel (exact only for 16-B/lane streaming reads)"
DECODE_PHASES = ("dec_plan", "decode", "dec_close")
KERNEL_SYMBOL["dec_plan"] = "k_dframe_count+k_scan_u32_u64+k_dframe_fill"


def roofline_whole_decode(kt, alg_bytes, profiled_shape: bool, whole=None):
    """(C + U) per step over the average time of the whole decode: `whole` = (ms, launches) of the
    timed steps' single span over the three phases (frame walk, block decode, verify); without it
    the summed averages of the phases' own event pairs."""
    parts = [p for p in DECODE_PHASES if p in kt] or (list(DECODE_PHASES) if whole else [])
    ms = whole[0] / whole[1] if whole else sum(kt[p][0] / kt[p][1] for p in parts)
    achieved = alg_bytes / (ms / 1e3) / 1e9
    traffic, tsrc = None, None
    if profiled_shape:
        tot = 0
        for p in parts:
            t, tsrc = pmc_traffic(p)
            if t is None:
                tot = None
                break
            tot += t
        traffic = tot
    roof = {
        "bound": "hbm", "kernel": "+".join(KERNEL_SYMBOL.get(p, p) for p in parts), "phases": parts,
        "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5),
        "traffic": traffic, "algorithmic_bytes_per_launch": alg_bytes, "avg_launch_ms": round(ms, 4),
    }
    if whole:
        roof["timed_in"] = "timed steps: one event pair over the three phases"
    if traffic is not None and tsrc:
        roof["traffic_source"] = tsrc + " (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE, same bench command)"
        roof["traffic_bound"] = TRAFFIC_BOUND
    return roof


def chunk_seed(rank: int, c: int) -> int:
    import synth
    return synth.SEED_BASE + 1 + 1000 * rank + 7919 * c


# ------------------------------------------------------------------ --dump-outputs
DUMP_SAMPLE = 1 << 20  # elements kept of each byte array (4 MiB as float32)
DUMP_SEED = 0x5EED0D0D


def _sample_bytes(buf, nbytes: int, tag: int):
    """float32 values of DUMP_SAMPLE bytes of buf[:nbytes] at seeded positions (the whole of a
    shorter array). The positions are fixed fractions of the length, so the shape is the same
    whatever nbytes is and two builds that write the same bytes dump the same array."""
    import numpy as np

    if nbytes <= DUMP_SAMPLE:
        return np.frombuffer(buf.read(nbytes), dtype=np.uint8).astype(np.float32)
    u = np.sort(np.random.default_rng(DUMP_SEED + tag).random(DUMP_SAMPLE))
    idx = np.minimum((u * nbytes).astype(np.int64), nbytes - 1)
    out = np.empty(DUMP_SAMPLE, dtype=np.float32)
    piece = 64 << 20  # read back 64 MiB at a time
    for lo in range(0, nbytes, piece):
        a, b = np.searchsorted(idx, [lo, lo + piece])
        if b > a:
            part = np.frombuffer(buf.read(min(piece, nbytes - lo), lo), dtype=np.uint8)
            out[a:b] = part[idx[a:b] - lo]
    return out


def dump_outputs(out_dir, rank, world, nb, block, d_frames, d_ioff, d_ilen, d_out, d_olen, d_ost):
    """What a caller of encode_dev + decode_dev receives from the last timed step, as float .npy
    files (about 8 MiB; rank r > 0 of a multi-GPU run adds `.rank<r>` to the names):
      frame_offsets, frame_lengths   float64[nb]  where the encoder put each frame, and its size
      decode_lengths, decode_status  float64[nb]  bytes decoded per frame, S3HC_* status per frame
      frames_sample                  float32      bytes of the packed frames at seeded positions
      decoded_sample                 float32      bytes of the decoded output at seeded positions
    Input and positions depend only on the arguments, so two builds compare array for array."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    fo = np.array(d_ioff.u64(nb), dtype=np.float64)
    fl = np.array(d_ilen.u32(nb), dtype=np.float64)
    comp = int(fo[-1] + fl[-1]) if nb else 0
    arrays = {
        "frame_offsets": fo,
        "frame_lengths": fl,
        "decode_lengths": np.array(d_olen.u32(nb), dtype=np.float64),
        "decode_status": np.array(d_ost.i32(nb), dtype=np.float64),
        "frames_sample": _sample_bytes(d_frames, min(comp, d_frames.numel()), 1),
        "decoded_sample": _sample_bytes(d_out, nb * block, 2),
    }
    suffix = f".rank{rank}" if world > 1 and rank else ""
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), a)
    return sorted(arrays)


def run_rank(args):
    import s3hc_lz4 as S
    import shard
    import synth

    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", os.environ.get("RANK", "0")))
    ndev = S.device_count()
    dev, why = assign_device(world, local, ndev, args.share_gpu)
    if dev is None:  # before any collective: the launcher kills the other ranks
        sys.stderr.write(f"bench.py: {why}\n")
        sys.exit(2)
    g = shard.Group()
    world, rank, local = g.world, g.rank, g.local
    block = 65536
    if args.total_blocks:
        lo, hi = shard.shard_range(args.total_blocks, world, rank)
        nb = hi - lo
    else:
        nb = args.blocks
    eng = S.Engine(dev)  # one process per GPU (devices shared only with --share-gpu)

    # ---- synthetic batch (distinct content, 256 MiB chunks), resident in HBM before timing
    nchunks = -(-nb // CHUNK_BLOCKS)
    d_src = eng.alloc(nb * block)
    first_chunk = None
    for c in range(nchunks):
        k = min(CHUNK_BLOCKS, nb - c * CHUNK_BLOCKS)
        part = synth.log_text(k * block, chunk_seed(rank, c))
        d_src.write(part, c * CHUNK_BLOCKS * block)
        if c == 0:
            first_chunk = part
    offs = [i * block for i in range(nb)]
    plan = eng.plan_encode(offs, [block] * nb)
    d_frames = eng.alloc(plan.dst_bound)
    d_ioff, d_ilen = eng.alloc(8 * nb), eng.alloc(4 * nb)
    d_out = eng.alloc(nb * block)
    d_olen, d_ost = eng.alloc(4 * nb), eng.alloc(4 * nb)

    # frame offsets are deterministic for a given input: learn them once for the decode plan
    eng.encode_dev(plan, d_src, d_frames, d_ioff, d_ilen)
    eng.sync()
    fo, fl = d_ioff.u64(nb), d_ilen.u32(nb)
    dplan = eng.plan_decode(fo, fl, offs, [block] * nb)
    comp_bytes = fo[-1] + fl[-1]

    # --pipeline: steps over two HIP queues, step k's decode (queue D) overlapping step k+1's
    # encode (queue E), which writes the other of two frame buffers; marks order enc(k) -> dec(k)
    # and dec(k) -> enc(k + 2). Every step still encodes and decodes its whole batch; the tail of
    # one kernel and the head of the next share the chip (+2.7 % per step), but the
    # kernels' own event spans then include the other queue's work, so the roofline durations are
    # not a kernel's own: the default stays one queue (serial), whose spans are.
    args.serial = not args.pipeline
    q_enc, q_dec = (None, None) if args.serial else (eng.queue(), eng.queue())
    frames = [d_frames] if args.serial else [d_frames, eng.alloc(plan.dst_bound)]
    ioffs = [d_ioff] if args.serial else [d_ioff, eng.alloc(8 * nb)]
    ilens = [d_ilen] if args.serial else [d_ilen, eng.alloc(4 * nb)]
    after_dec = {}
    nstep = [0]

    def step():
        i = nstep[0]
        nstep[0] += 1
        if args.serial:
            eng.encode_dev(plan, d_src, d_frames, d_ioff, d_ilen)
            eng.decode_dev(dplan, d_frames, d_out, d_olen, d_ost)
            return
        b = i & 1
        if i - 2 in after_dec:  # the decode that read this frame buffer is done
            m = after_dec.pop(i - 2)
            eng.wait_mark(m, q_enc)
            eng.free_mark(m)
        eng.encode_dev(plan, d_src, frames[b], ioffs[b], ilens[b], q_enc)
        m = eng.mark(q_enc)
        eng.wait_mark(m, q_dec)
        eng.free_mark(m)
        eng.decode_dev(dplan, frames[b], d_out, d_olen, d_ost, q_dec)
        after_dec[i] = eng.mark(q_dec)

    def sync_all():
        if not args.serial:
            q_enc.sync()
            q_dec.sync()
            for k in list(after_dec):
                if k < nstep[0] - 2:
                    eng.free_mark(after_dec.pop(k))
        eng.sync()

    for _ in range(args.warmup):
        step()
    sync_all()
    # correctness gate on the warmed-up state (outside the timed region)
    check = args.full and not args.skip_check
    if check:
        st = d_ost.i32(nb)
        assert st == [0] * nb, f"decode status {set(st)}"
        assert d_out.read(2 * block) == first_chunk[: 2 * block]

    # timed steps: HIP events only around the dominant kernel (k_enc_parse) and the whole decode
    # (coarse spans: every event record is a dispatch boundary, so fewer of them perturb the
    # timed region less); the per-phase breakdown comes from --profile-steps extra steps after it
    eng.timing_reset()
    eng.set_timing(not args.no_kernel_timing, coarse=True)
    g.barrier()
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    sync_all()
    t1 = time.perf_counter()
    g.barrier()
    eng.set_timing(False)
    elapsed = g.max(t1 - t0)
    kt_timed = eng.timing()
    dumped = None
    if args.dump_outputs:
        b = 0 if args.serial else (nstep[0] - 1) & 1  # the frame buffer the last timed step wrote
        dumped = dump_outputs(args.dump_outputs, rank, world, nb, block, frames[b], ioffs[b], ilens[b], d_out, d_olen, d_ost)
    kt = {}
    if args.full and not args.no_kernel_timing and args.profile_steps:
        eng.timing_reset()
        eng.set_timing(True)
        for _ in range(args.profile_steps):
            step()
        sync_all()
        eng.set_timing(False)
        kt = eng.timing()

    # full-output check after the timed steps: every block, every byte, chunk by chunk
    checked = 0
    if check:
        assert d_ost.i32(nb) == [0] * nb
        assert d_olen.u32(nb) == [block] * nb
        for c in range(nchunks):
            k = min(CHUNK_BLOCKS, nb - c * CHUNK_BLOCKS)
            want = first_chunk if c == 0 else synth.log_text(k * block, chunk_seed(rank, c))
            assert d_out.read(k * block, c * CHUNK_BLOCKS * block) == want, f"decoded chunk {c} differs from the input"
            checked += k
    checked_all = g.sum(float(checked))

    total_u = g.sum(float(nb * block)) * args.steps
    value = total_u / elapsed / GiB

    # ---- rooflines: the dominant kernel, and the decoder (north_star target)
    # side-stream spans overlap the match finder, so they never count as the dominant kernel
    excl = {k: v for k, v in kt.items() if not k.endswith("_side")}
    alg = {
        "enc_parse": nb * block,                  # U read once (match finding)
        "enc_emit": nb * block + comp_bytes,      # U literals read + C framed bytes written
        "decode": comp_bytes + nb * block,        # C read + U written
        "dec_close": nb * block,                  # U read (content xxh32 of every frame)
    }
    dom = max(excl, key=lambda k: excl[k][0] / excl[k][1]) if excl else None
    if not args.full and "enc_parse" in kt_timed:
        dom = "enc_parse"  # a plain run has no profiled steps: the one kernel its timed steps time by itself
    prof = nb == 4096 and not args.total_blocks
    # the dominant kernel's launch duration: from the timed steps' own events (enc_parse is timed
    # there), else from the profiled steps
    kdom = kt_timed if dom in kt_timed else kt
    roof = roofline_obj(kdom, dom, alg.get(dom, nb * block), prof) if dom else None
    if roof:
        roof["timed_in"] = "timed steps" if kdom is kt_timed else f"{args.profile_steps} profiled steps after the timed ones"
    # north_star decode figure over the whole decode the reference does in one FrameDecoder pass
    # (compression.rs:479-480): the plan's device frame walk, the block decode and the content
    # xxh32 verify + EndMark checks, timed as one span in the timed steps ("dec_all"); the phase
    # breakdown and the block-decode kernels alone come from the profiled steps
    roof_dec = None
    if "decode" in kt or (not args.full and "dec_all" in kt_timed):
        roof_dec = roofline_whole_decode(kt, alg["decode"], prof, kt_timed.get("dec_all"))
    roof_dec_k = roofline_obj(kt, "decode", alg["decode"], prof) if "decode" in kt else None
    per_kernel = {k: round(v[0] / v[1], 4) for k, v in kt.items()}
    rank_rate = nb * block * args.steps / (t1 - t0) / GiB
    rates, devs = [rank_rate], [dev]
    if g.dist is not None:
        import torch
        t = torch.tensor([rank_rate, float(dev)], dtype=torch.float64)
        lst = [torch.zeros(2, dtype=torch.float64) for _ in range(world)]
        g.dist.all_gather(lst, t)
        rates = [float(x[0].item()) for x in lst]
        devs = [int(x[1].item()) for x in lst]
    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(first_chunk, block, args.cpu_seconds)

    if rank == 0:
        line = {
            "metric": METRIC,
            "value": round(value, 3),
            "unit": "GiB/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "strong" if args.total_blocks else "weak",
            "vs_baseline": None,
            "dtype": "u8",
            "data": "synthetic S3 access-log text (SURVEY.md §8d config 2), seeded, every block distinct, distinct per rank",
            "config": {
                "workload": (f"config5: {args.total_blocks} x 64 KiB log-text blocks split over {world} GPUs" if args.total_blocks
                             else f"config2: {nb} x 64 KiB log-text blocks per GPU") + ", LZ4 frame encode + decode, device-resident",
                "blocks_per_gpu": nb, "block_bytes": block, "frame": "FLG 0x64 BD 0x40 (lz4_flex Auto), xxh32 content checksum",
                "compression_ratio": round(comp_bytes / (nb * block), 4), "parallelism": f"shard{world}",
                "queues": "pipelined (enc on E, dec on D)" if args.pipeline else "one queue, steps back to back",
                "decode_plan": "built before timing from the frame offsets/lengths the encoder wrote (read back once: "
                               "they are the same every step); the plan's frame walk (headers, block table, units) "
                               "runs on the device inside every timed step",
            },
            "per_gpu_gibps": [round(x, 3) for x in rates],
            "devices": {"visible": ndev, "rank_device": devs, "shared": len(set(devs)) < len(devs)},
            "full": args.full,
            "outputs_dumped": dumped,
            "blocks_checked": int(checked_all),
            "kernel_ms_per_step": per_kernel if args.full else None,
            "kernel_ms_source": (f"{args.profile_steps} steps after the timed ones, every phase its own event pair"
                                 if args.full else "not measured: --full times every phase"),
            "roofline": roof,
            "roofline_decode": roof_dec,
            "roofline_decode_kernels": roof_dec_k,
            "cpu_baseline": cpu,
        }
        print(json.dumps(line), flush=True)
    g.close()


def main():
    args = parse_args()
    rc = launch_decision(args)
    if rc is not None:
        sys.exit(rc)
    if args.selftest:
        selftest(args)
    else:
        run_rank(args)


if __name__ == "__main__":
    main()
