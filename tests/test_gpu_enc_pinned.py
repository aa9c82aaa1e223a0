"""Pinned encoder output. tests/enc_pinned.json holds the sha256 and the length of the frames the
match finder (csrc/s3hc_kernels.hip k_enc_parse<2,0> fast, <1,1> small) wrote for the seeded inputs
of tools/pin_frames.py before its vector-instruction cuts; every later build must write the same
bytes, and the frames must decode to their input with the oracle's decompress_data.

Cases (tools/pin_frames.py cases()): lengths at the segment edge, the prewarm tail, the group and
block boundaries and the last-12 / last-5 byte rules; log text; zeros (distance 1 + wave-wide
extension); periods 2..5; run starts without a table candidate (the distance-1..4 candidate on
single lanes); a repeated 1 KiB chunk (extensions past 256 bytes); random bytes; an 8-block batch."""
import hashlib
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import pin_frames  # noqa: E402

pytestmark = pytest.mark.gpu

with open(pin_frames.PINS) as _f:
    PINNED = json.load(_f)
CASES = pin_frames.cases()


def test_pins_cover_every_case():
    assert sorted(PINNED) == sorted(CASES)
    assert all(sorted(PINNED[c]) == sorted(pin_frames.MODES) for c in PINNED)


@pytest.mark.parametrize("mode", sorted(pin_frames.MODES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_frames_are_the_pinned_bytes(engine, oracle, name, mode):
    data, item = CASES[name]
    engine.set_encode_mode(pin_frames.MODES[mode])
    try:
        frames, fo, fl, offs, lens = pin_frames.encode(engine, data, item)
    finally:
        engine.set_encode_mode(0)
    want = PINNED[name][mode]
    assert len(frames) == want["length"], f"{name}/{mode}: frame bytes {len(frames)} != pinned {want['length']}"
    assert hashlib.sha256(frames).hexdigest() == want["sha256"], f"{name}/{mode}: frames differ from the pinned ones"
    mv = memoryview(data)
    for i in range(len(fo)):
        assert oracle.decompress_data(frames[fo[i]:fo[i] + fl[i]]) == mv[offs[i]:offs[i] + lens[i]], f"{name}/{mode} frame {i}"
