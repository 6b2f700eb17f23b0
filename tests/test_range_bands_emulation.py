"""The session loop of lep_decompress_batch_ranges stepped on the CPU (tests/emu/range_bands_emu.cc): the library's range plan, the
bookkeeping of lepton_amd/csrc/lep_stream_bands.h and lep_range_bands.h -- which segments a range touches, the window of every band, where
its bytes go, when a segment is retired, the checks and the tail at the end -- over the oracle's decoded frame, the decode faked band by
band, every band written by the emulated lane scan writer and copied through lep_pack.h's window_len and copy_run.

For ranges at every part boundary and 50 seeded random ones, at bands of 1 and 3 MCU rows and the doubling schedule: the answer must be
the file's bytes [first, first + len); the segments given to the session must be the plan's; at band 1 the last touched segment must be
retired behind exactly the first band at which its written count reaches its window's end (the per-band byte counts come from a whole
run of the same coder), and no other segment is retired; no byte outside a window is kept, on the host or in the answer."""
import ctypes as C
import json
import os
import random
import subprocess

import numpy as np
import pytest

import jpeg_writer as jw
import oracle_binding as ob
from conftest import GOLDEN, ROOT, golden
from lepton_amd import abi
from lepton_amd.codec import JpegImage, LepFile

FIXTURES = ["c420_odd_203x149", "q30_256x256_4seg", "rst_c420_176x112", "slice_4seg_q97", "gen_c420_4seg"]
MAXSEG = abi.MAX_SEGMENTS


class Report(C.Structure):
    _fields_ = [("advances", C.c_int32), ("nseg", C.c_int32), ("touched", C.c_int32 * MAXSEG), ("retired", C.c_int32 * MAXSEG),
                ("retire_advance", C.c_int32 * MAXSEG), ("rows_coded", C.c_int32 * MAXSEG), ("written", C.c_uint64 * MAXSEG),
                ("kept", C.c_uint64 * MAXSEG), ("host_bytes", C.c_uint64)]


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "range_bands_emu.cc")
    so = os.path.join(ROOT, "tests", "emu", "librange_bands_emu.so")
    tmp = "%s.%d" % (so, os.getpid())
    libdir = os.path.dirname(abi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, src, "-L" + libdir, "-llepton_mi355x", "-Wl,-rpath," + libdir])
    os.replace(tmp, so)
    abi.lib()
    L = C.CDLL(so)
    L.emu_range_bands.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_uint64, C.c_uint64, C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(Report)]
    L.emu_segment_row_bytes.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.c_int]
    return L


def generated_four_segments():
    """a dense 4:2:0 file of 560 x 400 that gets four thread segments, written through the oracle"""
    jpg, _ = jw.write_baseline(560, 400, [(1, 2, 2, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)], np.random.default_rng(9), density=0.9, amp=300.0, quality=50)
    src = JpegImage(jpg)
    streams, _ = ob.oracle_encode(src.desc, src.plan(8))
    return jpg, src.write_lep(streams, 8)


def plan_of(lep, first=0, length=0):
    rp = abi.RangePlan()
    assert abi.lib().lep_file_range_plan(lep, len(lep), first, length, C.byref(rp)) == 0
    return rp


def ranges_of(rp0, seed, randoms=50):
    """ranges at every part boundary (one byte on either side, the two bytes across, from each boundary to the next, both moved by one)
    and `randoms` seeded random ones"""
    size = rp0.jpeg_size
    edges = sorted({0, rp0.head_len, rp0.scan_bound, size} | {rp0.seg_first[q] + rp0.seg_len[q] for q in range(rp0.nseg)})
    out = [(0, 0), (0, size), (size - 1, 0)]
    for e in edges:
        out += [(e - 1, 1), (e, 1), (e - 1, 2), (e - 1, 0), (e, 0), (e + 1, 0)]
    for a, b in zip(edges, edges[1:]):
        out += [(a, b - a), (a + 1, b - a - 2), (a - 1, b - a + 2), (a, b - a + 1), (a + 1, b - a)]
    rnd = random.Random(seed)
    for _ in range(randoms):
        a = rnd.randrange(size)
        out.append((a, rnd.choice([1, 7, 512, 4096, 65536, rnd.randrange(1, size)])))
    return [(a, n) for a, n in dict.fromkeys(out) if 0 <= a < size and n >= 0]


@pytest.fixture(scope="module")
def files(emu):
    """per fixture, once: the restored bytes, the .lep, its parsed file with the oracle's frame in it, the whole-file plan, and per
    segment the cumulative byte counts of a run of the same coder one MCU row per band"""
    man = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    cache = {}

    def get(name):
        if name not in cache:
            if name.startswith("gen_"):
                want, lep = generated_four_segments()
            else:
                jpg, lep = golden(name)
                want = jpg[man[name]["slice"][0]:man[name]["slice"][1]] if "slice" in man[name] else jpg
            f = LepFile(lep)
            ob.oracle_decode(f.desc, f.segments, f.streams)
            rp0 = plan_of(lep)
            assert rp0.in_session == 1 and rp0.sizes_known == 1 and rp0.jpeg_size == len(want)
            if name.startswith("gen_"):
                assert rp0.nseg >= 3
            cum = []
            for q in range(rp0.nseg):
                buf = (C.c_uint64 * 4096)()
                n = emu.emu_segment_row_bytes(f.handle, q, buf, 4096)
                assert n > 0
                cum.append(list(buf[:n]))
            cache[name] = (want, lep, f, rp0, cum)
        return cache[name]

    return get


@pytest.mark.parametrize("band", [1, 3, 0])
@pytest.mark.parametrize("name", FIXTURES)
def test_ranges_are_the_files_bytes(emu, files, name, band):
    want, lep, f, rp0, cum = files(name)
    out = C.create_string_buffer(len(want) + 16)
    retired_somewhere = False
    for first, length in ranges_of(rp0, seed=len(want) + band):
        rp = plan_of(lep, first, length)
        if rp.first_seg < 0:   # the head alone: the call answers it from the header, no session
            assert rp.head_bytes == rp.length and rp.first + rp.length <= rp0.head_len
            continue
        rep, n = Report(), C.c_size_t(0)
        rc = emu.emu_range_bands(f.handle, lep, len(lep), first, length, band, out, len(want) + 16, C.byref(n), C.byref(rep))
        assert rc == 0, (first, length, rc)
        end = first + length if length else len(want)
        assert out.raw[:n.value] == want[first:end], (first, length)
        assert [q for q in range(rep.nseg) if rep.touched[q]] == list(range(rp.first_seg, rp.last_seg + 1)), (first, length)
        assert rep.host_bytes == 0
        for q in range(rp.first_seg, rp.last_seg + 1):
            skip, take = rp.win_skip[q], rp.win_take[q]
            assert rep.kept[q] == max(0, min(skip + take, rep.written[q]) - skip), (first, length, q)   # the window's bytes and no others
            if q != rp.last_seg:
                assert not rep.retired[q] and rep.written[q] == rp0.seg_len[q]
        q = rp.last_seg
        if band == 1:
            reach = next(k + 1 for k, c in enumerate(cum[q]) if c >= rp.win_skip[q] + rp.win_take[q]) if cum[q][-1] >= rp.win_skip[q] + rp.win_take[q] else None
            if reach is not None and reach < len(cum[q]):
                assert rep.retired[q] == 1 and rep.retire_advance[q] == reach and rep.written[q] == cum[q][reach - 1], (first, length)
            else:
                assert rep.retired[q] == 0 and rep.written[q] == cum[q][-1], (first, length)
        elif band == 0 and rep.retired[q]:   # the doubling schedule: 2^k - 1 rows after k advances, fewer than twice the rows needed
            need = next(k + 1 for k, c in enumerate(cum[q]) if c >= rp.win_skip[q] + rp.win_take[q])
            assert rep.retire_advance[q] == (need).bit_length() and 2 ** rep.retire_advance[q] - 1 < 2 * need
        retired_somewhere = retired_somewhere or bool(rep.retired[q])
        rows = max(len(cum[k]) for k in range(rp.first_seg, rp.last_seg + 1))
        assert rep.advances <= (-(-rows // band) if band > 0 else rows.bit_length() + 1)
    assert retired_somewhere
