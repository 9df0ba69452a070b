"""bench.py command line: the plain run stays lean (cpu_baseline is a --full
leg) and --dump-outputs writes the last timed step's outputs reproducibly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def test_bench_options_present():
    out = subprocess.run([sys.executable, BENCH, "--help"], check=True,
                         capture_output=True, text=True).stdout
    for opt in ("--full", "--dump-outputs", "--steps", "--warmup", "--gpus"):
        assert opt in out


def _run(outdir, *extra):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2",
                        "--warmup", "1", "--records", "20011",
                        "--dump-outputs", str(outdir), *extra],
                       check=True, capture_output=True, text=True, timeout=120)
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_dump_outputs_reproducible_and_consistent(tmp_path):
    import tez_amd
    if not tez_amd.device_available():
        pytest.skip("no GPU")
    n, rec = 20011, 4 + 16 + 4 + 64
    line = _run(tmp_path / "a")
    _run(tmp_path / "b")
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert line["cpu_baseline"] is None      # a --full leg only
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["counters.npy", "index.npy", "segment_crc32.npy",
                     "stream_sample.npy", "stream_sample_offsets.npy"]
    arrs = {}
    total_bytes = 0
    for nm in names:
        a = np.load(tmp_path / "a" / nm)
        b = np.load(tmp_path / "b" / nm)
        assert a.dtype in (np.float32, np.float64)
        assert a.shape == b.shape and np.array_equal(a, b), nm
        total_bytes += a.nbytes
        arrs[nm[:-4]] = a
    assert total_bytes <= 64e6
    # the dump is the step's real output: index identities + stream framing
    idx = arrs["index"]
    assert idx.shape == (64, 3)
    assert arrs["counters"][0] == n and arrs["counters"][1] == n * rec
    total = int(idx[-1, 0] + idx[-1, 2])
    assert np.array_equal(idx[1:, 0], np.cumsum(idx[:-1, 2]))
    # the stream is smaller than the sample: it is dumped whole
    stream = arrs["stream_sample"].astype(np.uint8).tobytes()[:total]
    assert arrs["stream_sample_offsets"][0] == 0 and len(stream) == total
    import zlib
    for p, (st, raw, cl) in enumerate(idx.astype(np.int64)):
        if cl == 0:
            continue
        seg = stream[st:st + cl]
        assert seg[:4] == b"TIF\x00" and cl == raw + 4
        assert zlib.crc32(seg[4:-4]) == int.from_bytes(seg[-4:], "big")
        assert arrs["segment_crc32"][p] == int.from_bytes(seg[-4:], "big")
