"""bench.py's plain and --full runs and --dump-outputs: the sampling of large byte arrays (CPU),
and on the GPU a small run of each kind whose dumped arrays must be the same, describe a clean
round trip of the seeded input, and whose lines carry what each kind of run measures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
NAMES = ["decode_lengths", "decode_status", "decoded_sample", "frame_lengths", "frame_offsets", "frames_sample"]


class _HostBuf:
    """DeviceBuffer's read() over host bytes."""

    def __init__(self, data):
        self.data, self.reads = data, []

    def read(self, n=None, offset=0):
        self.reads.append((n, offset))
        return self.data[offset:offset + n]


def test_sample_bytes_fixed_positions_and_shape(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench

    small = bytes(range(200))
    a = bench._sample_bytes(_HostBuf(small), len(small), 1)
    assert a.dtype == np.float32 and a.tolist() == list(range(200))  # short arrays are kept whole
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    data = np.random.default_rng(3).integers(0, 256, 300_001, dtype=np.uint8).tobytes()
    buf = _HostBuf(data)
    s1 = bench._sample_bytes(buf, len(data), 1)
    assert s1.dtype == np.float32 and s1.shape == (1000,)
    assert all(n + off <= len(data) for n, off in buf.reads)  # no read past the array
    assert np.array_equal(s1, bench._sample_bytes(_HostBuf(data), len(data), 1))  # same positions every time
    # every sampled value is the byte at its position: positions rise, so a ramp comes back sorted
    ramp = bytes((i * 256) // 300_001 for i in range(300_001))
    r = bench._sample_bytes(_HostBuf(ramp), len(ramp), 2)
    assert np.all(np.diff(r) >= 0) and r[0] <= 2 and r[-1] >= 253
    # one changed byte at a sampled position shows
    u = np.sort(np.random.default_rng(bench.DUMP_SEED + 1).random(1000))
    pos = int(u[500] * len(data))
    flipped = bytearray(data)
    flipped[pos] ^= 0xFF
    assert not np.array_equal(s1, bench._sample_bytes(_HostBuf(bytes(flipped)), len(data), 1))
    # a prefix of a longer buffer: only nbytes of it are sampled, the shape stays
    assert bench._sample_bytes(_HostBuf(data), 150_000, 1).shape == (1000,)


def _bench(args, timeout=120):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH] + args, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_same_outputs(tmp_path):
    import synth

    nb, block = 96, 65536
    common = ["--gpus", "1", "--blocks", str(nb), "--steps", "2", "--warmup", "1"]
    plain = _bench(common + ["--dump-outputs", str(tmp_path / "plain")])
    full = _bench(common + ["--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")])
    for d in (plain, full):
        assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["unit"] == "GiB/s" and d["dtype"] == "u8"
        assert d["higher_is_better"] is True and d["outputs_dumped"] == NAMES
        assert abs(d["value"] - nb * block / (d["ms_per_step"] / 1e3) / (1 << 30)) <= 0.01 * d["value"]
    # a plain run measures the steps alone; the checks and the per-phase steps are --full's
    assert plain["full"] is False and plain["kernel_ms_per_step"] is None and plain["cpu_baseline"] is None
    assert plain["blocks_checked"] == 0
    assert full["full"] is True and full["blocks_checked"] == nb and full["cpu_baseline"] is None
    assert {"enc_parse", "enc_emit", "decode", "dec_close"} <= set(full["kernel_ms_per_step"])
    assert full["roofline"] and full["roofline_decode"] and full["roofline_decode_kernels"]

    import bench
    data = synth.log_text(nb * block, bench.chunk_seed(0, 0))
    for name in NAMES:
        a, b = np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy")
        assert a.dtype in (np.float32, np.float64) and a.dtype == b.dtype
        assert np.array_equal(a, b), name
    out = {n: np.load(tmp_path / "plain" / f"{n}.npy") for n in NAMES}
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    assert np.all(out["decode_status"] == 0) and np.all(out["decode_lengths"] == block)
    fo, fl = out["frame_offsets"], out["frame_lengths"]
    assert fo[0] == 0 and np.array_equal(fo[1:], np.cumsum(fl)[:-1])  # frames packed back to back
    comp = int(fo[-1] + fl[-1])
    assert abs(comp / (nb * block) - plain["config"]["compression_ratio"]) < 1e-4
    # the decoded bytes at the sampled positions are the input's
    u = np.sort(np.random.default_rng(bench.DUMP_SEED + 2).random(bench.DUMP_SAMPLE))
    idx = np.minimum((u * nb * block).astype(np.int64), nb * block - 1)
    assert np.array_equal(out["decoded_sample"], np.frombuffer(data, dtype=np.uint8)[idx].astype(np.float32))
    # the packed frames are sampled too (their bytes are compared between builds, above)
    assert out["frames_sample"].shape == (min(comp, bench.DUMP_SAMPLE),)
    assert out["frames_sample"].min() >= 0 and out["frames_sample"].max() <= 255
