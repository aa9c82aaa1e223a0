"""Seekable range files on the GPU: the frame size scan (s3hc_frame_sizes_dev / s3hc_index_build),
the writer's index (s3hc_writer_commit_indexed) and the sliced read (s3hc_decompress_slice),
against the CPU oracle: len(oracle.decompress_data(frame)) and oracle.decompress_data(file)[lo:hi].
Shapes are the smallest that reach every path of the scan (one wave of segments, one chunk, several
chunks, several blocks, stored blocks, long length-extension runs)."""
import glob
import os
import random
import struct

import numpy as np
import pytest

import lz4ref
import synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KIB, MIB = 1 << 10, 1 << 20
K_FAST_MAX_C = 32768  # s3hc_plan.hpp kFastMaxC: the 64 KiB fast path's largest compressed block
K_LB_CHUNK = 8192     # s3hc_plan.hpp kLbChunk: the large-block tokenizer's chunk
K_SCAN_CHUNK = 16384  # s3hc_index.hip kChunk: the size scan's chunk (256 segments of 64 bytes)


def rnd(n, seed=1):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _block_csize(frame):
    """Compressed size of the first block of a frame without content size or dictionary id."""
    return struct.unpack_from("<I", frame, 7)[0] & 0x7FFFFFFF


def _log_frame_near(oracle, target, over):
    """A one-block frame of log text whose compressed block is the first one over `target` bytes
    (over) or the last one not over it, found by bisection on the input length."""
    text = synth.log_text(4 * target + 4096, 21)
    lo, hi = 1, len(text)  # csize(lo) <= target < csize(hi)
    assert len(oracle.lz4flex_compress_block(text[:hi])) > target
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if len(oracle.lz4flex_compress_block(text[:mid])) > target:
            hi = mid
        else:
            lo = mid
    frame = oracle.lz4flex_compress_frame(text[:hi if over else lo])
    c = _block_csize(frame)
    assert (target < c <= target + 16) if over else (target - 16 <= c <= target), (target, over, c)
    return frame


def _scan_cases(oracle):
    """[(name, frame)]: every frame decodes with the oracle."""
    cases = [
        ("empty", oracle.lz4flex_compress_frame(b"")),
        ("one_byte", oracle.lz4flex_compress_frame(b"x")),
        ("13_bytes", oracle.lz4flex_compress_frame(b"thirteen byte")),
        ("stored_random", oracle.lz4flex_compress_frame(rnd(3000, 2))),
        ("store_mode", oracle.store_mode_frame(rnd(70_000, 3))),
        ("zeros_64k", oracle.lz4flex_compress_frame(bytes(65536))),
        # a literal run of 70 000 bytes (its length-extension run is 274 bytes of 255: several
        # 64-byte walk segments) and a match run of 30 000 in one 256 KiB-BD frame
        ("rand70000_zeros30000", oracle.lz4flex_compress_frame(rnd(70_000, 4) + bytes(30_000))),
        ("under_fast_max", _log_frame_near(oracle, K_FAST_MAX_C, False)),
        ("over_fast_max", _log_frame_near(oracle, K_FAST_MAX_C, True)),  # (= over two scan chunks)
        ("over_one_lb_chunk", _log_frame_near(oracle, K_LB_CHUNK, True)),
        ("over_two_lb_chunks", _log_frame_near(oracle, 2 * K_LB_CHUNK, True)),  # (= over one scan chunk)
        ("under_one_scan_chunk", _log_frame_near(oracle, K_SCAN_CHUNK, False)),
        ("ref_1mib", oracle.lz4flex_compress_frame(synth.log_text(MIB, 99))),
        ("zeros_4mib", oracle.lz4flex_compress_frame(bytes(4 * MIB))),
        ("three_blocks_9mib", oracle.lz4flex_compress_frame(synth.log_text(9 * MIB, 5))),
    ]
    assert _block_csize(cases[3][1]) == 3000 and struct.unpack_from("<I", cases[3][1], 7)[0] >> 31  # stored block
    # liblz4's frames: linked blocks, block checksums, content size, block sizes 64 KiB .. 4 MiB
    for path in sorted(glob.glob(os.path.join(GOLDEN, "lz4f_*.lz4"))):
        cases.append((os.path.basename(path), open(path, "rb").read()))
    if lz4ref.available:
        d = synth.log_text(300_000, 8)
        for bsid in (4, 7):
            cases.append((f"liblz4_linked_bc_cs_{bsid}", lz4ref.compress_frame(d, bsid, True, True, True, True)))
            cases.append((f"liblz4_ind_{bsid}", lz4ref.compress_frame(d, bsid, False, False, False, False)))
    return cases


@pytest.fixture(scope="module")
def scan_cases(oracle):
    return _scan_cases(oracle)


def _scan(engine, frames):
    """(u_len, status) of every frame, one launch."""
    blob = b"".join(frames)
    off, o = [], 0
    for f in frames:
        off.append(o)
        o += len(f)
    n = len(frames)
    d_src = engine.upload(blob + bytes(16))
    d_len, d_st = engine.alloc(4 * n), engine.alloc(4 * n)
    d_len.fill(0xEE)
    d_st.fill(0xEE)
    engine.frame_sizes_dev(d_src, off, [len(f) for f in frames], d_len, d_st)
    return d_len.u32(n), d_st.i32(n)


def test_size_scan_matches_oracle(engine, oracle, scan_cases):
    want = [len(oracle.decompress_data(f)) for _, f in scan_cases]
    got, st = _scan(engine, [f for _, f in scan_cases])
    for (name, _), w, g, s in zip(scan_cases, want, got, st):
        print(f"{name}: oracle {w} scan {g} status {s}")
    assert st == [0] * len(scan_cases)
    assert got == want


def _corruptions(base, offs, n, seed):
    """n seeded corruptions of the frame chain `base` (frames start at offs), made as
    test_gpu_parity.py makes its own: a bit flip, a truncation, a byte, four bytes. Each is the
    one frame the change lands in (a truncation: that frame cut short)."""
    rng = random.Random(seed)
    ends = offs[1:] + [len(base)]
    out = []
    for t in range(n):
        b = bytearray(base)
        kind = t % 4
        if kind == 0:
            i = rng.randrange(len(b))
            b[i] ^= 1 << rng.randrange(8)
        elif kind == 1:
            i = rng.randrange(1, len(b))
            del b[i:]
        elif kind == 2:
            i = rng.randrange(11, len(b))
            b[i] = rng.randrange(256)
        else:
            i = rng.randrange(len(b))
            b[i:i + 4] = bytes(rng.randrange(256) for _ in range(4))
        k = max(j for j, o in enumerate(offs) if o <= min(i, len(b) - 1))
        out.append(bytes(b[offs[k]:len(b) if k + 1 == len(offs) else min(ends[k], len(b))]))
    return out


def _corrupt_frames(oracle):
    chain_frames = [oracle.lz4flex_compress_frame(synth.log_text(65536, 30 + k)) for k in range(4)]
    offs, o = [], 0
    for f in chain_frames:
        offs.append(o)
        o += len(f)
    frames = _corruptions(b"".join(chain_frames), offs, 60, 11)
    return frames + _corruptions(oracle.lz4flex_compress_frame(synth.log_text(MIB, 99)), [0], 40, 12)


def test_scan_agrees_with_decode(engine, oracle):
    import s3hc_lz4 as S

    frames = _corrupt_frames(oracle)
    u_len, st = _scan(engine, frames)
    passed = 0
    for f, u, s in zip(frames, u_len, st):
        if s != 0:  # the scan refused the frame
            assert u == 0
            continue
        passed += 1
        idx = S.FrameIndex.from_entries([len(f)], [u])
        d_st, d_out = engine.decompress_status(f)
        if d_st != 0:  # the decode fails: so does the sliced read of the whole frame
            if u:
                with pytest.raises(S.CodecError):
                    engine.read_slice(idx, f, 0, u)
            continue
        assert len(d_out) == u, "scan OK and decode OK with another length"
        assert d_out == oracle.decompress_data(f)
        assert engine.read_slice(idx, f, 0, u) == d_out
    print(f"{passed} of {len(frames)} corruptions passed the scan")
    # a scan that rejected everything would show nothing (checked on the CPU for these seeds:
    # the oracle alone decodes or checksum-fails more than 30 of the 100)
    assert passed >= 0.3 * len(frames)


@pytest.fixture(scope="module")
def sliced_file(engine, oracle):
    import s3hc_lz4 as S

    parts = [
        engine.compress_frame(synth.log_text(40 * 65536, 11), S.BLK_64K_PER_FRAME),
        engine.compress_frame(synth.log_text(MIB, 12)),  # Auto: one frame
        engine.store_mode_frame(rnd(50_000, 13)),
        engine.compress_frame(synth.log_text(5 * 65536, 14), S.BLK_64K_PER_FRAME),
    ]
    blob = b"".join(parts)
    plain = oracle.decompress_data(blob)
    assert len(plain) == 45 * 65536 + MIB + 50_000
    return blob, plain, engine.build_index(blob)


def test_build_index_of_mixed_file(sliced_file):
    blob, plain, idx = sliced_file
    assert [e[3] for e in idx.entries] == [65536] * 40 + [MIB, 50_000] + [65536] * 5
    assert idx.total == (len(blob), len(plain))


def test_sliced_read_matches_oracle(engine, sliced_file):
    blob, plain, idx = sliced_file
    n = len(plain)
    a, s, b = 40 * 65536, 40 * 65536 + MIB, 40 * 65536 + MIB + 50_000  # Auto frame, store-mode frame, tail
    slices = [(0, 0), (0, 1), (n - 1, n), (3 * 65536, 4 * 65536), (65536 - 1, 65536 + 1), (65536, 65536 + 1),
              (65536 - 1, 65536), (a + 123_457, a + 654_321), (s - 1000, b + 1000), (a - 1, b + 1), (0, n), (n, n)]
    for lo, hi in slices:
        assert engine.read_range(blob, idx, lo, hi) == plain[lo:hi], (lo, hi)
    # a one-frame slice reads that frame's bytes and no more: the file is not read whole
    first, count, c_off, c_len = idx.span(3 * 65536 + 5, 4 * 65536 - 5)
    assert (first, count) == (3, 1) and (c_off, c_len) == (idx.entries[3][0], idx.entries[3][2])
    assert c_len < 65536 and c_len < len(blob) // 40
    assert engine.read_slice(idx, blob[c_off:c_off + c_len], 3 * 65536 + 5, 4 * 65536 - 5) == plain[3 * 65536 + 5:4 * 65536 - 5]


@pytest.mark.parametrize("policy,compress,multi", [(0, True, False), (1, True, False), (2, True, False),
                                                   (0, False, False), (1, True, True)])
def test_writer_index_equals_built_index(engine, oracle, policy, compress, multi):
    import s3hc_lz4 as S

    data = synth.log_text(1_000_000, 40 + policy)
    agg = S.BatchAggregator([engine] if multi else engine, batch_size=256 * KIB, frame_policy=policy)
    try:
        w = agg.begin(0, len(data) - 1, compress)
        for i in range(0, len(data), 100_000):  # batches of 300 000 bytes: frames exceed batch_size
            w.write(data[i:i + 100_000])
        spec, idx = w.commit_indexed()
        blob = bytes(w.file)
    finally:
        agg.close()
    assert oracle.decompress_data(blob) == data
    assert (spec.compressed_size, spec.uncompressed_size) == (len(blob), len(data)) == idx.total
    want_frames = 3 * 5 + 2 if policy == 1 and compress else 4
    assert len(idx) == want_frames
    assert idx == engine.build_index(blob)
    assert S.FrameIndex.from_bytes(idx.to_bytes()) == idx
    assert engine.read_range(blob, idx, 299_990, 300_010) == data[299_990:300_010]  # across two batches


def test_slice_faults(engine, oracle):
    import s3hc_lz4 as S

    data = synth.log_text(10 * 65536, 50)
    blob = engine.compress_frame(data, S.BLK_64K_PER_FRAME)
    idx = engine.build_index(blob)
    ent = idx.entries
    assert len(ent) == 10

    def fails(status, index, span, lo, hi, msg=None, **kw):
        with pytest.raises(S.CodecError) as e:
            engine.read_slice(index, span, lo, hi, **kw)
        assert e.value.status == status, e.value
        if msg:
            assert msg in str(e.value)

    # a content-checksum byte of frame 7: slices touching it fail whole, earlier frames still read
    bad = bytearray(blob)
    bad[ent[7][0] + ent[7][2] - 1] ^= 0x40
    bad = bytes(bad)
    for lo, hi in ((7 * 65536 + 10, 7 * 65536 + 20), (6 * 65536, 8 * 65536), (0, len(data))):
        f, k, co, cl = idx.span(lo, hi)
        fails(S.S3HC_CHECKSUM, idx, bad[co:co + cl], lo, hi)
    assert engine.read_range(bad, idx, 0, 7 * 65536) == data[:7 * 65536]
    # an index with one u_len off by one
    c, u = [e[2] for e in ent], [e[3] for e in ent]
    for d in (1, -1):
        forged = S.FrameIndex.from_entries(c, u[:4] + [u[4] + d] + u[5:])
        lo, hi = forged.entries[4][1], forged.entries[4][1] + forged.entries[4][3]
        f, k, co, cl = forged.span(lo, hi)
        fails(S.S3HC_CORRUPT, forged, blob[co:co + cl], lo, hi, "stale index")
    # a span shifted by one byte
    lo, hi = 2 * 65536, 4 * 65536
    f, k, co, cl = idx.span(lo, hi)
    fails(S.S3HC_CORRUPT, idx, blob[co + 1:co + cl + 1], lo, hi)
    fails(S.S3HC_CORRUPT, idx, blob[co - 1:co + cl - 1], lo, hi)
    fails(S.S3HC_CORRUPT, idx, blob[co:co + cl - 1], lo, hi, "stale index")
    # a destination one byte short
    fails(S.S3HC_DST_TOO_SMALL, idx, blob[co:co + cl], lo, hi, cap=hi - lo - 1)
    assert engine.read_slice(idx, blob[co:co + cl], lo, hi) == data[lo:hi]
    # an empty frame in the middle ends the index, as it ends decompress_data
    cut = ent[3][0]
    mid = blob[:cut] + oracle.lz4flex_compress_frame(b"") + blob[cut:]
    assert oracle.decompress_data(mid) == data[:3 * 65536]
    short = engine.build_index(mid)
    assert short.entries == ent[:3] and short.total == (cut, 3 * 65536)
