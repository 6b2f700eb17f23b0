"""bench.py --dump-outputs on the MI355X: the last timed step's outputs as .npy files (float32 / float64, under 64 MB in all),
the same arrays from two runs with the same arguments -- what lets two builds of the project be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(out_dir, steps):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--images", "24", "--unique", "3",
           "--width", "640", "--height", "480", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_dump_outputs_are_the_same_from_run_to_run(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    out = run(a, 3)
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and "mixed" not in out and "end_to_end" not in out
    run(b, 2)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and all(n.endswith(".npy") for n in names)
    assert {"encode_stream_lengths.npy", "encode_stream_crc32.npy", "encode_stream_bytes_sample.npy", "decode_status.npy",
            "decode_frame_crc32.npy", "decode_coefficients_sample.npy"} <= set(names)
    assert sum(os.path.getsize(a / n) for n in names) <= 64 << 20
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64), n
        assert x.shape == y.shape and np.array_equal(x, y), n
    assert not np.load(a / "decode_status.npy").any()
    lens = np.load(a / "encode_stream_lengths.npy")
    assert len(lens) == out["config"]["segments_per_gpu"] and (lens > 0).all()
    assert np.load(a / "decode_frame_crc32.npy").shape[0] == 3
    assert np.abs(np.load(a / "decode_coefficients_sample.npy")).sum() > 0
