"""The band loop of lep_decompress_batch_stream stepped on the CPU (tests/emu/stream_bands_emu.cc): the bookkeeping of
lepton_amd/csrc/lep_stream_bands.h -- the rows a band adds to every thread segment, the state its writer starts from, where its bytes are
appended, which bytes may go out -- over the oracle's decoded frame, the decode faked band by band from the segments' row ranges and every
band written by the emulated lane scan writer.  The pieces must concatenate to the JPEG, no byte of a segment may go out before the segment
in front of it is complete, and a writer whose byte bound is too small must end in the host re-coder with the same bytes."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
from conftest import ROOT, golden
from lepton_amd import abi
from lepton_amd.codec import JpegImage, LepFile

PIECE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_size_t)
FIXTURES = ["c420_odd_203x149", "q30_256x256_4seg", "rst_c420_176x112", "gen_c422_rst7"]


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "stream_bands_emu.cc")
    so = os.path.join(ROOT, "tests", "emu", "libstream_bands_emu.so")
    tmp = "%s.%d" % (so, os.getpid())
    libdir = os.path.dirname(abi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, src, "-L" + libdir, "-llepton_mi355x", "-Wl,-rpath," + libdir])
    os.replace(tmp, so)
    abi.lib()
    L = C.CDLL(so)
    L.emu_stream_bands.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, PIECE_FN, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    return L


def _generated_422():
    """4:2:2, 792 x 480 (the smallest of its kind that gets two thread segments): 50 MCUs per row, restart interval 7 -- an interval ends
    where an MCU row does only every seventh row"""
    from PIL import Image

    rng = np.random.default_rng(422)
    base = np.asarray(Image.fromarray(rng.integers(0, 256, (60, 99, 3), dtype=np.uint8), "RGB").resize((792, 480), Image.BICUBIC)).astype(np.int16)
    pic = Image.fromarray(np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8), "RGB")
    buf = io.BytesIO()
    pic.save(buf, format="JPEG", quality=88, subsampling="4:2:2", restart_marker_blocks=7)
    return buf.getvalue()


@pytest.fixture(scope="module")
def files():
    """per fixture, once: (the JPEG, its parsed .lep with the oracle's decoded frame in it, the planned segments' MCU rows)"""
    cache = {}

    def get(name):
        if name not in cache:
            if name.startswith("gen_"):
                jpg = _generated_422()
                src = JpegImage(jpg)
                streams, _ = ob.oracle_encode(src.desc, src.plan(4))
                lep = src.write_lep(streams, 4)
            else:
                jpg, lep = golden(name)
            f = LepFile(lep)
            ob.oracle_decode(f.desc, f.segments, f.streams)
            img, segs = abi.HuffImage(), (abi.HuffSegment * abi.MAX_SEGMENTS)()
            nseg, ok = C.c_int(0), C.c_int(0)
            assert abi.lib().lep_file_recode_plan(f.handle, C.byref(img), segs, C.byref(nseg), C.byref(ok)) == 0 and ok.value
            if name.startswith("gen_"):
                assert img.rsti == 7 and img.mcuh % img.rsti and nseg.value > 1
            cache[name] = (jpg, f, [(segs[q].mcu_row0, segs[q].mcu_row1) for q in range(nseg.value)])
        return cache[name]

    return get


def run(emu, f, band, shrink_seg=-1, shrink_cap=0):
    pieces = []

    def piece(_user, seg, advance, data, n):
        pieces.append((seg, advance, C.string_at(data, n)))
        return 0

    declined, advances = C.c_int32(0), C.c_int32(0)
    rc = emu.emu_stream_bands(f.handle, band, shrink_seg, shrink_cap, PIECE_FN(piece), None, C.byref(declined), C.byref(advances))
    return rc, pieces, declined.value, advances.value


def complete_after(rows, band, advance):
    """is a segment of MCU rows [r0, r1) complete after `advance` advances of the faked decode?"""
    r0, r1 = rows
    return band <= 0 or r0 + advance * band >= r1


@pytest.mark.parametrize("band", [1, 3, 0])
@pytest.mark.parametrize("name", FIXTURES)
def test_pieces_are_the_file_and_segments_go_out_in_order(emu, files, name, band):
    jpg, f, rows = files(name)
    rc, pieces, declined, advances = run(emu, f, band)
    assert rc == 0 and not declined
    assert b"".join(p for _, _, p in pieces) == jpg
    longest = max(r1 - r0 for r0, r1 in rows)
    assert advances == (1 if band <= 0 else -(-longest // band))
    assert pieces[0][0] == -1 and pieces[0][1] == 0, "the header goes out before the first advance"
    order = [s for s, _, _ in pieces if s >= 0]
    assert order == sorted(order)
    for seg, advance, _ in pieces:
        if seg >= 1:
            assert all(complete_after(rows[q], band, advance) for q in range(seg)), (seg, advance)
    if band == 1 and rows[0][1] - rows[0][0] > 2:
        first = [a for s, a, _ in pieces if s == 0]
        assert first[0] == 1 and len(first) > 2, "the front segment goes out as its rows come"


@pytest.mark.parametrize("band", [1, 3, 0])
@pytest.mark.parametrize("name", FIXTURES)
def test_writer_bound_too_small_ends_in_the_host_recoder(emu, files, name, band):
    jpg, f, rows = files(name)
    last = len(rows) - 1
    for seg, cap in ((0, 40), (last, 9)):
        rc, pieces, declined, _ = run(emu, f, band, seg, cap)
        assert rc == 0 and declined
        assert b"".join(p for _, _, p in pieces) == jpg
