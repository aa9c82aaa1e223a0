#!/usr/bin/env python3
"""Pins the encoder's output: sha256 and length of the frames the loaded library writes for a
fixed set of seeded inputs, in both encode modes (tests/enc_pinned.json; tests/test_gpu_enc_pinned.py
asserts them). A change to the match finder that must not alter frames is run against the pins of
the commit before it.

Usage: [S3HC_LIB_PATH=...] python tools/pin_frames.py            print the table
       [S3HC_LIB_PATH=...] python tools/pin_frames.py --write    rewrite tests/enc_pinned.json
       ... --check                                                 compare with tests/enc_pinned.json
"""
import hashlib
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINS = os.path.join(ROOT, "tests", "enc_pinned.json")
BLOCK = 65536
# segment edge, prewarm tail positions 4093..4095, group boundary, block boundary, and the
# last-12-bytes / last-5-bytes rules
LENGTHS = (12, 13, 4095, 4096, 4097, 8192 + 5, 32768 + 5, 65536, 65536 + 13)
MODES = {"fast": 0, "small": 1}


def _repeat(unit: bytes, n: int) -> bytes:
    return (unit * (n // len(unit) + 1))[:n]


def cases() -> dict:
    """name -> (data, item length). One item per case except "batch" (8 items of one block)."""
    import synth

    rng = random.Random(0x5EED08)
    out = {}
    for n in LENGTHS:
        out[f"len_{n}"] = (synth.log_text(n, synth.SEED_BASE + 80), n)
    out["log"] = (synth.log_text(3 * BLOCK + 1234, synth.SEED_BASE + 81), 3 * BLOCK + 1234)
    out["zeros"] = (bytes(BLOCK + 4097 + 7), BLOCK + 4097 + 7)
    for p in (2, 3, 4, 5):
        unit = bytes(rng.sample(range(256), p))
        out[f"period{p}"] = (_repeat(unit, 20000 + p), 20000 + p)
    # run starts where the table has no candidate: 37 random bytes then 40 equal ones
    runs = b"".join(rng.randbytes(37) + bytes([rng.randrange(256)]) * 40 for _ in range(2 * BLOCK // 77 + 1))
    out["runstarts"] = (runs[: 2 * BLOCK - 9], 2 * BLOCK - 9)
    out["chunk1k"] = (_repeat(rng.randbytes(1024), BLOCK + 30000), BLOCK + 30000)
    out["random"] = (rng.randbytes(BLOCK + 5000), BLOCK + 5000)
    out["batch"] = (synth.log_text(8 * BLOCK, synth.SEED_BASE + 82), BLOCK)
    return out


def encode(engine, data: bytes, item: int):
    """The frames of data cut into items (device path); -> (bytes, frame offsets, frame lengths, item offsets, item lengths)."""
    n = max(1, -(-len(data) // item))
    offs = [i * item for i in range(n)]
    lens = [min(item, len(data) - o) for o in offs]
    d_src = engine.upload(data)
    plan = engine.plan_encode(offs, lens)
    dst = engine.alloc(plan.dst_bound)
    ioff, ilen = engine.alloc(8 * n), engine.alloc(4 * n)
    engine.encode_dev(plan, d_src, dst, ioff, ilen)
    engine.sync()
    fo, fl = ioff.u64(n), ilen.u32(n)
    return dst.read(fo[-1] + fl[-1]), fo, fl, offs, lens


def pins(engine) -> dict:
    out = {}
    try:
        for name, (data, item) in cases().items():
            out[name] = {}
            for mname, mode in MODES.items():
                engine.set_encode_mode(mode)
                frames = encode(engine, data, item)[0]
                out[name][mname] = {"sha256": hashlib.sha256(frames).hexdigest(), "length": len(frames)}
    finally:
        engine.set_encode_mode(0)
    return out


def main() -> int:
    sys.path[:0] = [os.path.join(ROOT, "sample-s3-hybrid-cache_amd")]
    import s3hc_lz4 as S

    got = pins(S.Engine(0))
    text = json.dumps(got, indent=1, sort_keys=True) + "\n"
    if "--write" in sys.argv:
        with open(PINS, "w") as f:
            f.write(text)
        print(f"wrote {PINS}: {len(got)} cases x {len(MODES)} modes")
    elif "--check" in sys.argv:
        with open(PINS) as f:
            want = json.load(f)
        bad = [f"{c}/{m}" for c in want for m in want[c] if got.get(c, {}).get(m) != want[c][m]]
        print("frames differ: " + ", ".join(bad) if bad else f"all {len(want) * len(MODES)} pinned frames identical")
        return 1 if bad else 0
    else:
        sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
