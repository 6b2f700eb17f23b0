"""lep_gpu_rgb_device's wavefront routine (lepton_amd/csrc/lep_rgb.h: wave_rgb and the record table in front of it) stepped through the
64-lane emulation on the CPU (tests/emu/rgb_emu.cc), as a program of its own built with AddressSanitizer and UBSan, on the images of
tests/rgb_cases.py: every layout (4:4:4, 4:2:2, 4:2:0, 4:4:0, 4:1:1, an upsampled luma, two kinds of chroma in one frame, components as
they are, one component), widths 1..8 and round a unit's 256 pixels, heights 1, 2, 3 and 17, three kinds of pitch, row ranges, several
images in one table.  Planes and outputs are heap blocks of exactly their size.  Every pixel must equal tests/rgb_ref.py, and every byte
of an output that is not a pixel of a requested row must be untouched."""
import os
import struct
import subprocess

import numpy as np
import pytest

import rgb_cases
from conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("rgb_emu")
    exe = str(tmp_path / "rgb_emu")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-Wall", "-Werror", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "emu", "rgb_emu.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True)      # (no fallback: a compiler without the sanitizers' runtimes fails these tests)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def pad3(v):
    return list(v) + [1] * (3 - len(v))


def run(exe, tmp_path, tables):
    blob = [struct.pack("<i", len(tables))]
    for _, images in tables:
        blob.append(struct.pack("<i", len(images)))
        for m in images:
            n = len(m["planes"])
            blob.append(struct.pack("<16i", m["width"], m["height"], n, int(m["convert"]), *pad3(m["h_samp"]), *pad3(m["v_samp"]),
                                    *(list(m["plane_pitch"]) + [0] * (3 - n)), m["rgb_pitch"], *m["rows"]))
            blob.extend(m["planes"])
    (tmp_path / "cases.bin").write_bytes(b"".join(blob))
    r = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout, r.stderr[-3000:])
    raw = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=np.uint8)
    at = 0
    for name, images in tables:
        for m in images:
            n = (m["height"] - 1) * m["rgb_pitch"] + m["row_bytes"]
            got, want = raw[at:at + n], rgb_cases.expected(m, n)
            assert np.array_equal(got, want), (name, m["width"], m["height"], m["rows"], m["plane_pitch"], m["rgb_pitch"], int((got != want).sum()))
            at += n
    assert at == len(raw)
    return int(r.stdout.split()[1])


def test_lanes_equal_the_definition(exe, tmp_path):
    tables = rgb_cases.tables()
    assert {m["layout"] for _, t in tables for m in t} == set(rgb_cases.LAYOUTS)
    ran = run(exe, tmp_path, tables)
    assert ran == sum(rgb_cases.units(m) for _, t in tables for m in t)


def test_an_image_the_definition_refuses_has_no_record(exe, tmp_path):
    """2 x 1 chroma in a frame whose largest factor is 3: no integral factor"""
    blob = struct.pack("<2i16i", 1, 1, 8, 8, 3, 1, 3, 2, 1, 1, 1, 1, 8, 8, 8, 24, 0, 8)
    (tmp_path / "cases.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3, (r.returncode, r.stderr[-2000:])
