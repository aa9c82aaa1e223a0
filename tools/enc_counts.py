#!/usr/bin/env python3
"""Event counts of the match finder from a diagnostic build (S3HC_DIAG_LEVEL=11): one encode of
the config-2 batch (4096 x 64 KiB log text) per encode mode, then per 4 KiB segment: steps, the
steps that ran the distance-1..4 candidate block and how many lanes wanted it, walk landings,
hops and wave-wide extensions.
Usage: make -C sample-s3-hybrid-cache_amd diag DIAG=-DS3HC_DIAG_LEVEL=11 TAG=cnt
       S3HC_LIB_PATH=.../build/diag/lib_cnt.so python tools/enc_counts.py [zeros]"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sample-s3-hybrid-cache_amd")]
import s3hc_lz4 as S  # noqa: E402
import synth  # noqa: E402

NAMES = ["segments", "steps", "short_steps", "short_1", "short_2", "short_3", "short_4_7", "short_8_15",
         "short_16_31", "short_32_64", "short_lanes", "landings", "hops", "extensions"]


def main():
    nb, block = int(os.environ.get("PROF_BLOCKS", "4096")), 65536
    eng = S.Engine(0)
    f = ctypes.CDLL(S.LIB_PATH).s3hc_diag_enc_counts
    f.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
    buf = (ctypes.c_ulonglong * 16)()
    data = bytes(nb * block) if "zeros" in sys.argv else synth.log_text(nb * block, synth.SEED_BASE + 1)
    offs = [i * block for i in range(nb)]
    d_src = eng.upload(data)
    plan = eng.plan_encode(offs, [block] * nb)
    d_frames = eng.alloc(plan.dst_bound)
    d_ioff, d_ilen = eng.alloc(8 * nb), eng.alloc(4 * nb)
    out = {}
    for mname, mode in (("fast", S.ENC_FAST), ("small", S.ENC_SMALL)):
        eng.set_encode_mode(mode)
        f(buf, 16, 1)
        eng.encode_dev(plan, d_src, d_frames, d_ioff, d_ilen)
        eng.sync()
        f(buf, 16, 0)
        v = list(buf)
        segs = v[0] or 1
        out[mname] = {"total": dict(zip(NAMES, v)), "per_segment": {n: round(x / segs, 2) for n, x in zip(NAMES, v)}}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
