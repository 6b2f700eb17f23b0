"""The band loop of lep_decompress_batch_stream stepped on the CPU (tests/emu/stream_layouts_emu.cc) over the layouts that the streamed calls
take besides whole interleaved files: one-component files -- the writer's rows are block rows, lepton_amd/csrc/lep_stream_bands.h converts --,
-startbyte / -trunc slices, and files cut inside their scan, whose last segment ends where its writer meets the cut with the byte bound
reached.  Every one of them must finish on the writer (declined == 0) with the bytes lep_file_recode gives; a slot smaller than the bound
and a cut met in front of the bound must end in the host re-coder with the same bytes.  And the rule itself, lep_file_streams_in_session."""
import ctypes as C
import os
import subprocess

import pytest

import oracle_binding as ob
from conftest import GOLDEN, ROOT, golden
from lepton_amd import abi
from lepton_amd.codec import LepFile
from stream_layout_cases import FIXTURES, GENERATED, NOT_STREAMED, lep_of

PIECE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint8), C.c_size_t)
NAMES = list(FIXTURES) + [GENERATED]


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "stream_layouts_emu.cc")
    so = os.path.join(ROOT, "tests", "emu", "libstream_layouts_emu.so")
    tmp = "%s.%d" % (so, os.getpid())
    libdir = os.path.dirname(abi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, src, "-L" + libdir, "-llepton_mi355x", "-Wl,-rpath," + libdir])
    os.replace(tmp, so)
    abi.lib()
    L = C.CDLL(so)
    L.emu_stream_layouts.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_uint32, PIECE_FN, C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.emu_planned_rows_per_mcu_row.argtypes = [C.c_void_p]
    return L


@pytest.fixture(scope="module")
def files(emu):
    """per file, once: (what lep_file_recode gives, its parsed .lep with the oracle's decoded frame in it, the planned segments' MCU rows
    -- planned rows over the product's planned rows per MCU row, a short last MCU row rounded up)"""
    cache = {}

    def get(name):
        if name not in cache:
            f = LepFile(lep_of(name))
            ob.oracle_decode(f.desc, f.segments, f.streams)
            want = f.recode()
            img, segs = abi.HuffImage(), (abi.HuffSegment * abi.MAX_SEGMENTS)()
            nseg, ok = C.c_int(0), C.c_int(0)
            assert abi.lib().lep_file_recode_plan(f.handle, C.byref(img), segs, C.byref(nseg), C.byref(ok)) == 0 and ok.value
            unit = emu.emu_planned_rows_per_mcu_row(f.handle)
            assert unit >= 1
            if name == GENERATED:
                assert img.ncomp == 1 and nseg.value >= 2
            if name == "lay_gray22_80x56":
                assert unit == 2 and segs[nseg.value - 1].mcu_row1 % 2 == 1, "two block rows per MCU row, the last MCU row short"
            if name == "slice_4seg_q97":
                assert nseg.value == 4
            for q in range(nseg.value):
                assert segs[q].mcu_row0 % unit == 0
            cache[name] = (want, f, [(segs[q].mcu_row0 // unit, -(-segs[q].mcu_row1 // unit)) for q in range(nseg.value)])
        return cache[name]

    return get


def run(emu, f, band, shrink_seg=-1, shrink_cap=0, grow_last=0):
    pieces = []

    def piece(_user, seg, advance, data, n):
        pieces.append((seg, advance, C.string_at(data, n)))
        return 0

    declined, advances = C.c_int32(0), C.c_int32(0)
    rc = emu.emu_stream_layouts(f.handle, band, shrink_seg, shrink_cap, grow_last, PIECE_FN(piece), None, C.byref(declined), C.byref(advances))
    return rc, pieces, declined.value, advances.value


def complete_after(rows, band, advance):
    """is a segment of MCU rows [r0, r1) complete after `advance` advances of the faked decode?"""
    r0, r1 = rows
    return band <= 0 or r0 + advance * band >= r1


def test_golden_slices_and_cut_files_restore_what_they_were_made_from(files):
    """lep_file_recode, the reference of everything below, against the golden JPEGs: a whole file is the .jpg, a slice a part of it"""
    for name, kind in FIXTURES.items():
        want = files(name)[0]
        jpg = golden(name)[0]
        assert (want in jpg) if "slice" in kind else (want == jpg), name


@pytest.mark.parametrize("band", [1, 3, 0])
@pytest.mark.parametrize("name", NAMES)
def test_pieces_are_the_file_without_the_host_recoder(emu, files, name, band):
    want, f, rows = files(name)
    rc, pieces, declined, advances = run(emu, f, band)
    assert rc == 0
    assert declined == 0
    assert b"".join(p for _, _, p in pieces) == want
    longest = max(r1 - r0 for r0, r1 in rows)
    assert advances == (1 if band <= 0 else max(1, -(-longest // band)))
    if pieces[0][0] == -1:
        assert pieces[0][1] == 0, "the header goes out before the first advance"
    assert all(s != -1 for s, _, _ in pieces[1:])
    order = [s for s, _, _ in pieces if s >= 0]
    assert order == sorted(order)
    for seg, advance, _ in pieces:
        if seg >= 1:
            assert all(complete_after(rows[q], band, advance) for q in range(seg)), (seg, advance)
    if band == 1 and rows[0][1] - rows[0][0] > 2:
        first = [a for s, a, _ in pieces if s == 0]
        assert first[0] == 1 and len(first) > 2, "the front segment goes out as its rows come"


@pytest.mark.parametrize("band", [1, 3, 0])
@pytest.mark.parametrize("name", ["gray_120x88", "slice_tail_q97", "truncated", "slice_4seg_q97", GENERATED])
def test_slot_smaller_than_the_bound_ends_in_the_host_recoder(emu, files, name, band):
    want, f, rows = files(name)
    last = len(rows) - 1
    for seg, cap in ((0, 40), (last, 9)):
        rc, pieces, declined, _ = run(emu, f, band, seg, cap)
        assert rc == 0 and declined
        assert b"".join(p for _, _, p in pieces) == want


@pytest.mark.parametrize("band", [1, 3, 0])
@pytest.mark.parametrize("name", ["truncated", "slice_mid_q97"])
def test_cut_met_in_front_of_the_bound_declines(emu, files, name, band):
    """the last segment's byte bound (and slot) 1000 bytes beyond the plan's: its writer meets the cut with the bound not reached"""
    want, f, _ = files(name)
    rc, pieces, declined, _ = run(emu, f, band, grow_last=1000)
    assert rc == 0 and declined == 1
    assert b"".join(p for _, _, p in pieces) == want


def test_the_rule():
    q = abi.lib().lep_file_streams_in_session
    for name in NAMES:
        lep = lep_of(name)
        assert q(lep, len(lep)) == 1, name
    for name in NOT_STREAMED:
        lep = golden(name)[1]
        assert q(lep, len(lep)) == 0, name
    # a chained pair: two files of format version 2 (only those mark their end) back to back -- each alone is streamed
    one = open(os.path.join(GOLDEN, "v2", "c420_160x120.lep"), "rb").read()
    assert LepFile(one + one).more
    assert q(one, len(one)) == 1 and q(one + one, 2 * len(one)) == 0
    for junk in (b"", b"\x00" * 64, b"not a lepton file at all, not even close" * 4, lep_of("gray_120x88")[:20]):
        assert q(junk, len(junk)) > 1, junk
