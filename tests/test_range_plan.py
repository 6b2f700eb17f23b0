"""lep_file_range_plan (lepton_amd/csrc/lep_range.h): where a byte range of the restored file lies -- head, one extent per thread
segment, tail.  Host only.  The test reads the hand-offs itself, from the HH section of the container's zlib header, and walks the JPEG's
markers for the head; the plan's extents must be contiguous from head_len, every segment but the last must have its hand-off's
segment_size, and for ranges at every part boundary +-1 the touched segments, the windows and the head's share must be what the
extents say.  The last segment's length is "to the tail" and flagged as not known from the header; its window is open to where the
garbage starts, and a range that reaches behind its first byte touches it even where it lies in the tail."""
import ctypes as C
import json
import os
import struct
import zlib

import pytest

from conftest import GOLDEN, golden
from lepton_amd import abi

FIXTURES = ["q30_256x256_4seg", "slice_4seg_q97", "gray_120x88", "truncated", "rst_c420_176x112", "prog_c420_320x240"]


def header_sections(lep):
    """the sections of a format-1 container's header: {marker: payload}; HH -> [segment_size per hand-off]"""
    assert lep[:2] == b"\xcf\x84" and lep[2] == 1
    jpeg_size, zsize = struct.unpack_from("<II", lep, 20)
    p = zlib.decompress(lep[28:28 + zsize])
    assert p[:3] == b"HDR"
    hdrs = struct.unpack_from("<I", p, 3)[0]
    out = {"jpeg_size": jpeg_size, "HDR": p[7:7 + hdrs]}
    pos = 7 + hdrs
    assert p[pos:pos + 3] in (b"P0D", b"PAD")
    pos += 4
    while pos + 3 <= len(p):
        m = p[pos:pos + 3]
        pos += 3
        if m[:2] == b"HH":
            n = m[2]
            out["HH"] = [struct.unpack_from("<I", p, pos + 16 * k + 2)[0] for k in range(n)]
            pos += 16 * n
        elif m == b"CRS":
            pos += 4 + 4 * struct.unpack_from("<I", p, pos)[0]
        elif m in (b"FRS", b"GRB", b"PGR", b"PGE"):
            c = struct.unpack_from("<I", p, pos)[0]
            out[m.decode()] = p[pos + 4:pos + 4 + c]
            pos += 4 + c
        elif m == b"SIZ":
            out["jpeg_size"] = struct.unpack_from("<I", p, pos)[0]
            pos += 4
        elif m == b"EEE":
            pos += 28
        else:
            break
    return out


def head_of_jpeg(jpg):
    """bytes in front of the scan: SOI and every marker segment up to and including the first SOS header"""
    pos = 2
    while True:
        assert jpg[pos] == 0xFF
        n = 2 + struct.unpack_from(">H", jpg, pos + 2)[0]
        if jpg[pos + 1] == 0xDA:
            return pos + n
        pos += n


def plan(lep, first=0, length=0):
    rp = abi.RangePlan()
    assert abi.lib().lep_file_range_plan(lep, len(lep), first, length, C.byref(rp)) == 0
    return rp


@pytest.fixture(scope="module")
def cases():
    man = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    out = {}
    for name in FIXTURES:
        jpg, lep = golden(name)
        restored = jpg[man[name]["slice"][0]:man[name]["slice"][1]] if "slice" in man[name] else jpg
        out[name] = (jpg, lep, restored, header_sections(lep))
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_extents_are_the_headers(cases, name):
    jpg, lep, restored, sec = cases[name]
    rp = plan(lep)
    assert rp.in_session == abi.lib().lep_file_streams_in_session(lep, len(lep))
    assert rp.jpeg_size == sec["jpeg_size"] == len(restored)
    assert (rp.first, rp.length) == (0, len(restored))
    if name.startswith("prog_"):
        assert rp.in_session == 0 and rp.nseg == 0 and (rp.first_seg, rp.last_seg, rp.head_bytes) == (-1, -1, 0)
        return
    sizes = sec["HH"]
    assert rp.in_session == 1 and rp.nseg == len(sizes) and rp.sizes_known == 1 and rp.last_len_known == 0
    if "PGR" in sec:   # a -startbyte / -trunc file counts in its own bytes: its head is the prefix garbage
        assert rp.head_len == len(sec["PGR"]) and restored[:rp.head_len] == sec["PGR"]
    else:
        assert rp.head_len == head_of_jpeg(jpg)
    at = rp.head_len
    for q in range(rp.nseg):
        assert rp.seg_first[q] == at
        if q + 1 < rp.nseg:
            assert rp.seg_len[q] == sizes[q]
        at += rp.seg_len[q]
    garbage = sec.get("GRB", b"\xff\xd9")
    assert rp.tail_len >= len(garbage) and at + rp.tail_len == rp.jpeg_size
    assert rp.scan_bound == rp.jpeg_size - len(garbage) and restored.endswith(garbage)
    assert (rp.first_seg, rp.last_seg, rp.head_bytes) == (0, rp.nseg - 1, rp.head_len)


def test_hand_derived_extents(cases):
    rp = plan(cases["q30_256x256_4seg"][1])
    assert (rp.head_len, rp.nseg, rp.jpeg_size, rp.tail_len) == (623, 2, 178322, 2)
    assert list(rp.seg_len)[:2] == [88562, 89135]
    rp = plan(cases["slice_4seg_q97"][1])
    assert rp.jpeg_size == 310000 and rp.nseg == 4
    assert list(rp.seg_len)[:3] == [71208, 71337, 80555]
    assert rp.seg_len[3] + rp.tail_len == 78640   # (the slice's last two bytes are its garbage)


def expected(rp0, first, length):
    """from the extents alone: (first, length, head_bytes, first_seg, last_seg, {q: (skip, take)})"""
    size = rp0.jpeg_size
    if first >= size:
        return size, 0, 0, -1, -1, {}
    length = size - first if length == 0 or length > size - first else length
    end = first + length
    head = max(0, min(end, rp0.head_len) - first)
    wins = {}
    for q in range(rp0.nseg):
        s0 = rp0.seg_first[q]
        last = q + 1 == rp0.nseg
        s1 = max(s0, min(size, rp0.scan_bound)) if last else s0 + rp0.seg_len[q]
        lo, hi = max(first, s0), min(end, s1)
        if (end > s0) if last else (hi > lo):
            wins[q] = (min(lo, s1) - s0, max(hi - lo, 0))
    return first, length, head, min(wins, default=-1), max(wins, default=-1), wins


@pytest.mark.parametrize("name", [n for n in FIXTURES if not n.startswith("prog_")])
def test_ranges_at_every_part_boundary(cases, name):
    lep = cases[name][1]
    rp0 = plan(lep)
    edges = [0, rp0.head_len] + [rp0.seg_first[q] + rp0.seg_len[q] for q in range(rp0.nseg)] + [rp0.scan_bound, rp0.jpeg_size]
    points = sorted({e + d for e in edges for d in (-1, 0, 1) if 0 <= e + d <= rp0.jpeg_size + 1})
    checked = 0
    for a in points:
        for b in points:
            if b <= a:
                continue
            for length in (b - a, 0):
                rp = plan(lep, a, length)
                first, ln, head, fs, ls, wins = expected(rp0, a, length)
                assert (rp.first, rp.length, rp.head_bytes, rp.first_seg, rp.last_seg) == (first, ln, head, fs, ls), (a, length)
                assert {q: (rp.win_skip[q], rp.win_take[q]) for q in range(rp.nseg) if q in wins} == wins, (a, length)
                assert rp.reaches_last == (1 if rp0.nseg - 1 in wins else 0)
                # the head's share and the windows' inside the extents cover the range up to the last segment's start
                inside = head + sum(t for q, (s, t) in wins.items() if q + 1 < rp0.nseg)
                assert inside == max(0, min(first + ln, rp0.seg_first[rp0.nseg - 1]) - first)
                checked += 1
    assert checked > 50


def test_clipping_and_the_empty_answer(cases):
    lep = cases["q30_256x256_4seg"][1]
    size = 178322
    rp = plan(lep, size - 10, 1000)
    assert (rp.first, rp.length) == (size - 10, 10) and (rp.first_seg, rp.last_seg) == (1, 1)
    for first in (size, size + 1, 1 << 40):
        rp = plan(lep, first, 5)
        assert rp.length == 0 and (rp.first_seg, rp.last_seg, rp.head_bytes) == (-1, -1, 0)
    rp = plan(lep, 0, (1 << 64) - 1)
    assert (rp.first, rp.length) == (0, size)
    rp = plan(lep, 100, 200)   # inside the head: no segment
    assert (rp.first_seg, rp.last_seg, rp.head_bytes) == (-1, -1, 200)
    # a file that does not parse answers its exit code
    rp = abi.RangePlan()
    bad = abi.lib().lep_file_range_plan(b"\xcf\x84" + bytes(40), 42, 0, 0, C.byref(rp))
    assert bad != 0 and bad == abi.lib().lep_file_open(b"\xcf\x84" + bytes(40), 42, C.byref(C.c_void_p()))
