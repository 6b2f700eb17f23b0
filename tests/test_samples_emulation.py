"""lep_gpu_samples_device's wavefront routines (lepton_amd/csrc/lep_samples.h: wave_samples, wave_samples_dc and the record table in
front of them) stepped through the 64-lane emulation on the CPU (tests/emu/samples_emu.cc), as a program of its own built with
AddressSanitizer and UBSan: the frames of tests/samples_frames.py -- every row width that takes another path through a unit of eight
blocks, random coefficients inside the domain, the domain's corners --, at both scales, whole planes and row ranges, several planes in
one table.  Frames, planes and the LDS tile are heap blocks of exactly their size.  Every sample must equal tests/samples_ref.py, and
every byte of a plane's buffer that is not a sample of a requested row must be untouched.  For the frames outside the domain only the
sanitizers' silence and the untouched bytes are checked."""
import os
import struct
import subprocess

import numpy as np
import pytest

import samples_frames as sf
from conftest import ROOT


def build(tmp_path):
    exe = str(tmp_path / "samples_emu")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-o", exe, os.path.join(ROOT, "tests", "emu", "samples_emu.cc")]
    if subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-o", str(tmp_path / "probe"), "-"], input="int main() { return 0; }\n",
                      capture_output=True, text=True).returncode != 0:
        cmd = [c for c in cmd if not c.startswith("-fsanitize") and not c.startswith("-fno-sanitize")]   # no sanitizer runtime: the byte checks alone
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run(exe, tmp_path, cases):
    """cases: [(scale, [(q, blocks, (row_first, row_end), pitch)])] -> per case and plane the buffer the program wrote"""
    blob = [struct.pack("<i", len(cases))]
    for scale, planes in cases:
        blob.append(struct.pack("<ii", scale, len(planes)))
        for q, blocks, rows, pitch in planes:
            blob.append(struct.pack("<5i", blocks.shape[1], blocks.shape[0], rows[0], rows[1], pitch))
            blob.append(np.asarray(q, dtype="<u2").tobytes())
            blob.append(np.ascontiguousarray(blocks, dtype="<i2").tobytes())
    (tmp_path / "cases.bin").write_bytes(b"".join(blob))
    r = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr[-3000:])
    raw = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.uint8)
    out, at = [], 0
    for scale, planes in cases:
        got = []
        for q, blocks, rows, pitch in planes:
            h, w = sf.plane_size(blocks, scale)
            n = (h - 1) * pitch + w
            got.append(raw[at:at + n])
            at += n
        out.append(got)
    assert at == len(raw)
    return out, int(r.stdout.split()[1])


def units(blocks, rows, scale):
    return (rows[1] - rows[0]) * ((blocks.shape[1] + (63 if scale == 8 else 7)) // (64 if scale == 8 else 8))


def check(cases, got, compare=True):
    for (scale, planes), bufs in zip(cases, got):
        for (q, blocks, rows, pitch), buf in zip(planes, bufs):
            want = sf.expected_rows(q, blocks, scale, rows, pitch).reshape(-1)[:len(buf)]
            if compare:
                assert np.array_equal(buf, want), (scale, blocks.shape, rows, pitch, int((buf != want).sum()))
            else:
                outside = sf.expected_rows(q, np.zeros_like(blocks), scale, rows, pitch).reshape(-1)[:len(buf)] == sf.CANARY   # (zero frame: every sample is 128)
                assert (buf[outside] == sf.CANARY).all(), (scale, blocks.shape, rows, pitch)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("samples_emu"))


def test_lanes_equal_the_definition_inside_the_domain(exe, tmp_path):
    cases = []
    for name, q, blocks in sf.in_domain():
        h, w = blocks.shape[:2]
        for scale in (1, 8):
            width = w * 8 // scale
            cases.append((scale, [(q, blocks, (0, h), width)]))                      # planes with no slack at all
            cases.append((scale, [(q, blocks, (0, h), width + 24)]))
            if h >= 3:
                cases.append((scale, [(q, blocks, (1, h - 1), width)]))              # a range in the middle
                cases.append((scale, [(q, blocks, (1, 1), width)]))                  # an empty one
                cases.append((scale, [(q, blocks, (0, 1), width + 3)]))              # two that together are the whole (odd pitch: byte stores)
                cases.append((scale, [(q, blocks, (1, h), width + 3)]))
    # several planes in one table: different geometry, a plane without units between two with
    frames = {n: (q, b) for n, q, b in sf.in_domain()}
    for scale in (1, 8):
        planes = []
        for n, rows, extra in (("random_17x3", (0, 3), 0), ("random_9x3", (2, 2), 0), ("random_1x1", (0, 1), 24), ("corners", (0, 11), 0), ("random_8x3", (1, 3), 8)):
            q, b = frames[n]
            planes.append((q, b, rows, b.shape[1] * 8 // scale + extra))
        cases.append((scale, planes))
    got, ran = run(exe, tmp_path, cases)
    assert ran == sum(units(b, rows, scale) for scale, planes in cases for _, b, rows, _ in planes)
    check(cases, got)


def test_frames_outside_the_domain_stay_in_bounds_and_overflow_nothing(exe, tmp_path):
    cases = []
    for name, q, blocks in sf.outside_domain():
        h, w = blocks.shape[:2]
        for scale in (1, 8):
            cases.append((scale, [(q, blocks, (0, h), w * 8 // scale)]))
            cases.append((scale, [(q, blocks, (1, h), w * 8 // scale + 24)]))
    got, _ = run(exe, tmp_path, cases)
    check(cases, got, compare=False)
