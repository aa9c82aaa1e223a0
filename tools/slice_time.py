#!/usr/bin/env python3
"""Timing of the seekable-range-file paths on one GPU.

  scan64k   size scan (s3hc_frame_sizes_dev) of 4096 x 64 KiB frames of log text, against the
            whole device decode of the same frames ("dec_all": plan walk + decode + close)
  scan1m    the same for 256 x 1 MiB frames (one 1 MiB block each, the reference's cache format)
  slice     sliced read of 1 MiB at random offsets of a 256 MiB object in 64 KiB frames (host
            buffers: s3hc_index_span + s3hc_decompress_slice), against s3hc_decompress_frames of
            the whole file followed by a slice

Each step runs in a child process of its own (one at a time) under its own time limit; this
process never opens the GPU, and stops at the first step that fails. Device times are HIP event
spans (s3hc_set_timing), host times a wall clock around calls that return synchronised; every
figure is the median of --runs runs, the two sides of a comparison alternating. One JSON object
on stdout (and in --out).
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sample-s3-hybrid-cache_amd")]

MiB = 1 << 20
STEPS = {"scan64k": 180, "scan1m": 180, "slice": 420}  # seconds allowed per step


def scan_step(n, item, runs, reps):
    import s3hc_lz4 as S
    import synth

    eng = S.Engine(0)
    data = synth.log_text(n * item, synth.SEED_BASE + 1)
    offs = [i * item for i in range(n)]
    d_src = eng.upload(data)
    plan = eng.plan_encode(offs, [item] * n)
    d_fr = eng.alloc(plan.dst_bound)
    d_io, d_il = eng.alloc(8 * n), eng.alloc(4 * n)
    eng.encode_dev(plan, d_src, d_fr, d_io, d_il)
    eng.sync()
    fo, fl = d_io.u64(n), d_il.u32(n)
    comp = fo[-1] + fl[-1]
    d_out = eng.alloc(n * item + 64)
    d_ol, d_os = eng.alloc(4 * n), eng.alloc(4 * n)
    d_ul, d_us = eng.alloc(4 * n), eng.alloc(4 * n)
    dp = eng.plan_decode(fo, fl, offs, [item] * n)
    # warm up and check both
    eng.decode_dev(dp, d_fr, d_out, d_ol, d_os)
    eng.frame_sizes_dev(d_fr, fo, fl, d_ul, d_us)
    eng.sync()
    ok = d_os.i32(n) == [0] * n and d_ol.u32(n) == [item] * n and d_us.i32(n) == [0] * n and d_ul.u32(n) == [item] * n
    dec, scan = [], []
    eng.set_timing(True, coarse=True)
    for _ in range(runs):
        eng.timing_reset()
        for _ in range(reps):
            eng.decode_dev(dp, d_fr, d_out, d_ol, d_os)
        eng.sync()
        dec.append(eng.timing()["dec_all"][0] / reps)
        eng.timing_reset()
        for _ in range(reps):
            eng.frame_sizes_dev(d_fr, fo, fl, d_ul, d_us)
        eng.sync()
        scan.append(eng.timing()["size_scan"][0] / reps)
    eng.set_timing(False)
    d, s = statistics.median(dec), statistics.median(scan)
    return {"frames": n, "frame_bytes": item, "compressed_bytes": comp, "check": ok, "runs": runs, "reps": reps,
            "dec_all_ms": round(d, 4), "dec_all_runs_ms": [round(x, 4) for x in dec],
            "size_scan_ms": round(s, 4), "size_scan_runs_ms": [round(x, 4) for x in scan],
            "scan_over_decode": round(s / d, 4), "scan_compressed_GBps": round(comp / s / 1e6, 1),
            # what a launch stores, from its shape: u_len and status per frame, nothing per chunk or block
            "scan_bytes_written": 8 * n}


def slice_step(runs):
    import s3hc_lz4 as S
    import synth

    eng = S.Engine(0)
    total, want = 256 * MiB, MiB
    data = synth.log_text(total, synth.SEED_BASE + 1)
    blob = eng.compress_frame(data, S.BLK_64K_PER_FRAME)
    t0 = time.perf_counter()
    idx = eng.build_index(blob)
    t_index = time.perf_counter() - t0
    assert idx.total == (len(blob), total) and len(idx) == total // 65536
    out_all = ctypes.create_string_buffer(total)
    out_sl = ctypes.create_string_buffer(want)
    n = ctypes.c_size_t()
    rng = random.Random(5)
    whole, sliced, frames, ok = [], [], [], True
    for r in range(runs + 1):  # (the first pair warms both paths up and is dropped)
        lo = rng.randrange(0, total - want)
        hi = lo + want
        t0 = time.perf_counter()
        rc = S.lib.s3hc_decompress_frames(eng.h, blob, len(blob), out_all, total, ctypes.byref(n))
        ref = out_all[lo:hi]
        t1 = time.perf_counter()
        first, count, c_off, c_len = idx.span(lo, hi)
        span = blob[c_off:c_off + c_len]  # (the caller's read of the file)
        rc2 = S.lib.s3hc_decompress_slice(eng.h, idx.h, first, count, span, c_len, lo, hi, out_sl, want, ctypes.byref(n))
        got = out_sl.raw
        t2 = time.perf_counter()
        ok = ok and rc == 0 and rc2 == 0 and got == ref == data[lo:hi]
        if r:
            whole.append((t1 - t0) * 1e3)
            sliced.append((t2 - t1) * 1e3)
            frames.append(count)
    w, s = statistics.median(whole), statistics.median(sliced)
    return {"object_bytes": total, "file_bytes": len(blob), "slice_bytes": want, "check": ok, "runs": runs,
            "frames_touched": frames, "index_build_ms": round(t_index * 1e3, 2), "index_sidecar_bytes": len(idx.to_bytes()),
            "whole_decode_then_slice_ms": round(w, 3), "whole_runs_ms": [round(x, 3) for x in whole],
            "sliced_read_ms": round(s, 3), "sliced_runs_ms": [round(x, 3) for x in sliced],
            "whole_over_sliced": round(w / s, 1)}


def child(step, runs):
    if step == "scan64k":
        res = scan_step(4096, 65536, runs, 20)
    elif step == "scan1m":
        res = scan_step(256, MiB, runs, 10)
    else:
        res = slice_step(runs)
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", default=",".join(STEPS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.runs)
        return 0
    out = {}
    for step in args.steps.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step, "--runs", str(args.runs)],
                               capture_output=True, text=True, timeout=STEPS[step])
        except subprocess.TimeoutExpired:
            out[step] = {"error": f"no result within {STEPS[step]} s"}
            break  # (nothing more is started on the GPU after a step that did not end)
        line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            out[step] = {"error": f"exit {r.returncode}", "stderr": r.stderr[-2000:]}
            break
        out[step] = json.loads(line[-1][7:])
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0 if all("error" not in v for v in out.values()) and len(out) == len(args.steps.split(",")) else 1


if __name__ == "__main__":
    sys.exit(main())
