"""The stitched bool writer with its chunks cut at the boundaries of gather's parts (lep_enc5.h part_chunk_cut / wchunk_range_cut /
wchunk_link_cuts / wchunk_code_cut, one wchunk_stitch_lane over all parts x chunks) stepped on the CPU, part by part as the GPU launches
it (tests/emu/enc5_part_chunks_emu.cc) -- a program of its own built with AddressSanitizer and UBSan: random and adversarial bin lists
cut at random part bounds against the serial coder, and whole segments of the frames of tests/enc5_gather_frames.py through count ->
emit -> fold -> gather in parts -> the per-part chunk phases against the oracle's streams."""
import ctypes as C
import os
import struct
import subprocess

import pytest

import oracle_binding as ob
from conftest import ROOT
from enc5_gather_frames import CONTENTS, frame
from lepton_amd import abi

# the GPU test's shapes (segments of 1, 2 and a few tiles a row) and two whose segments have fewer tiles than parts
SHAPES = [(64, 4, False), (65, 2, False), (129, 4, False), (65, 3, True), (1, 3, True), (63, 2, False)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("enc5_part_chunks")
    out = str(d / "enc5_part_chunks")
    # (-fwrapv: the walks' IDCT multiplies the dense frames' 11-bit coefficients past 32 bits and wraps, as the reference's does; the
    # writer is this test's subject)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fwrapv", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-o", out, os.path.join(ROOT, "tests", "emu", "enc5_part_chunks_emu.cc")]
    if subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-o", str(d / "probe"), "-"], input="int main() { return 0; }\n",
                      capture_output=True, text=True).returncode != 0:
        cmd = [c for c in cmd if not c.startswith("-fsanitize") and not c.startswith("-fno-sanitize")]   # no sanitizer runtime: the byte checks alone
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _clean(r):
    return r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_bin_lists_cut_at_random_part_bounds_equal_the_serial_writer(exe):
    """1 .. 8 parts of 1 / 2 / 4 / 8 chunks, empty parts, parts of a few bins, warm-ups from 8 bins to longer than the list, buffers too
    small; the link pass must have redone chunks in some trials and none in others"""
    r = subprocess.run([exe, "lists", "3000"], capture_output=True, text=True, timeout=300)
    assert _clean(r) and r.stdout.startswith("ok lists 3000 "), (r.stdout, r.stderr[-3000:])
    said = dict(zip(r.stdout.split()[3::2], map(int, r.stdout.split()[4::2])))
    assert said["with_redo"] > 100 and said["without_redo"] > 100, said
    assert said["empty_parts"] > 100 and said["short_parts"] > 100 and said["overflows"] >= 30, said


def test_whole_segments_in_parts_equal_the_oracle(exe, tmp_path):
    files = []
    for shape in SHAPES:
        for content in CONTENTS:
            img = frame(*shape, content)
            plan = img.plan()
            assert len(plan) == 1
            want, _ = ob.oracle_encode(img.desc, plan)
            d, s = img.desc, plan[0]
            fn = tmp_path / ("%dx%d_%d_%s.frame" % (shape[0], shape[1], shape[2], content))
            with open(fn, "wb") as f:
                f.write(C.string_at(C.addressof(d), abi.ImageDesc.blocks.offset))
                for c in range(d.ncomp):
                    f.write(C.string_at(d.blocks[c], d.nblocks(c) * 128))
                f.write(struct.pack("<iiiI", s.luma_y_start, s.luma_y_end, s.is_last, len(want[0])))
                f.write(want[0])
            files.append(str(fn))
    r = subprocess.run([exe, "frames"] + files, capture_output=True, text=True, timeout=300)
    assert _clean(r) and r.stdout.startswith("ok frames %d runs %d " % (len(files), 12 * len(files))), (r.stdout, r.stderr[-3000:])
    assert int(r.stdout.split()[8]) == len(files)   # every frame was also refused for want of room (status 100)
