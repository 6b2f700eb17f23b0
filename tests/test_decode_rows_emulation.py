"""The resumable decoder (lep_dec4.h Dec4WaveT::run_rows, the body of lep_decode_v4_rows_kernel) stepped on the CPU band after band
(tests/emu/dec_rows_emu.cc): a segment decoded in bands of MCU rows -- a fresh wave object and fresh LDS for every band, only the model,
the summary rings, the frame, the resume record and the saved LDS Branches carried over -- must give what the one-shot decoder and the
oracle give, must say truthfully after every band which block rows are in the frame, and must name the block at which a damaged stream
turned inconsistent, with everything in front of that block stored and nothing behind it touched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
from conftest import ROOT, golden
from lepton_amd import abi
from lepton_amd.codec import JpegImage

FILL = 0x5A
FIXTURES = ["one_block_8x8", "one_col_8x64", "one_col_420_16x80", "gray_120x88", "c444_96x80", "c420_odd_203x149", "truncated",
            "truncated_short", "q30_256x256_4seg", "lay_440_640x480_2seg"]
AFTER_BAND = C.CFUNCTYPE(None, C.c_void_p, C.c_int)


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "dec_rows_emu.cc")
    so = os.path.join(ROOT, "tests", "emu", "libcore_emu_decrows.so")
    tmp = "%s.%d" % (so, os.getpid())
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, src])
    os.replace(tmp, so)
    L = C.CDLL(so)
    L.emu_decode_segment_v4_rows_watched.argtypes = [C.POINTER(abi.ImageDesc), C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_uint32, C.c_int,
                                                     C.POINTER(abi.DecodeProgress), C.c_int, C.POINTER(C.c_uint32), AFTER_BAND, C.c_void_p]
    L.emu_decode_segment_v4_rows.argtypes = L.emu_decode_segment_v4_rows_watched.argtypes[:10]
    return L


def fill_frame(d):
    for c in range(d.ncomp):
        C.memset(d.blocks[c], FILL, d.nblocks(c) * 128)


def frame_of(d):
    """the frame as one (rows, width, 128) byte array per component"""
    return [np.frombuffer(C.string_at(d.blocks[c], d.nblocks(c) * 128), dtype=np.uint8).reshape(d.height_blocks[c], d.width_blocks[c], 128).copy()
            for c in range(d.ncomp)]


def segment_rows(d, s, c):
    """the block rows of component c that segment s codes"""
    m0, mc = d.height_blocks[0] // d.mcu_rows, d.height_blocks[c] // d.mcu_rows
    first = s.luma_y_start // m0 * mc
    last = d.coded_height[c] if s.is_last else min(s.luma_y_end // m0 * mc, d.coded_height[c])
    return first, max(first, last)


def segment_mcu_rows(d, s):
    m0 = d.height_blocks[0] // d.mcu_rows
    first, last = segment_rows(d, s, 0)
    return -(-last // m0) - first // m0


@pytest.fixture(scope="module")
def decoded():
    """per fixture, once: (image, segments, the oracle's streams, its bin count, the oracle's frame decoded into a FILL-ed frame)"""
    cache = {}

    def get(name):
        if name not in cache:
            img = JpegImage(golden(name)[0])
            segs = img.plan()
            streams, bins = ob.oracle_encode(img.desc, segs)
            fill_frame(img.desc)
            ob.oracle_decode(img.desc, segs, streams)
            cache[name] = (img, segs, streams, bins, frame_of(img.desc))
        return cache[name]

    return get


@pytest.mark.parametrize("band", [1, 2, 3, 0])
@pytest.mark.parametrize("name", FIXTURES)
def test_banded_decode_equals_one_shot_decode(emu, decoded, name, band):
    img, segs, streams, bins, oracle_frame = decoded(name)
    d = img.desc
    # the one-shot emulation (core_emu.cc is part of the driver's library) into a FILL-ed frame: the frame every band is held against
    fill_frame(d)
    total = 0
    for s, w in zip(segs, streams):
        nb = C.c_uint32(0)
        assert emu.emu_decode_segment_v4(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, w, len(w), C.byref(nb)) == 0
        total += nb.value
    final = frame_of(d)
    assert total == bins
    for c in range(d.ncomp):
        assert np.array_equal(final[c], oracle_frame[c]), "one-shot emulation and oracle disagree"

    fill_frame(d)
    banded_bins = 0
    for s, w in zip(segs, streams):
        nrows = segment_mcu_rows(d, s)
        prog = (abi.DecodeProgress * (nrows + 2))()
        seen = []
        problems = []

        def after_band(_user, k):
            p = prog[k]
            now = frame_of(d)
            if seen and any(p.rows_done[c] < seen[-1][c] for c in range(d.ncomp)):
                problems.append("band %d: rows_done went down" % k)
            seen.append([p.rows_done[c] for c in range(d.ncomp)])
            for c in range(d.ncomp):
                first, last = segment_rows(d, s, c)
                done = p.rows_done[c]
                if done and not first <= done - 1 < max(last, first + 1):
                    problems.append("band %d: rows_done[%d] = %d outside the segment's rows %d..%d" % (k, c, done, first, last))
                lo = max(first, min(done, last))
                if not np.array_equal(now[c][first:lo], final[c][first:lo]):
                    problems.append("band %d: a row of component %d below rows_done is not final" % (k, c))
                if not (now[c][lo:last] == FILL).all():
                    problems.append("band %d: a row of component %d at or above rows_done is not untouched" % (k, c))

        nb = C.c_uint32(0)
        n = emu.emu_decode_segment_v4_rows_watched(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, w, len(w), band, prog, nrows + 2, C.byref(nb),
                                                   AFTER_BAND(after_band), None)
        assert not problems, problems[:4]
        assert n == (1 if band == 0 else -(-nrows // band)), (n, nrows)
        assert [prog[k].status for k in range(n)] == [-1] * (n - 1) + [0]
        assert all(prog[k].fail_component == prog[k].fail_y == prog[k].fail_x == -1 for k in range(n))
        for c in range(d.ncomp):
            first, last = segment_rows(d, s, c)
            assert prog[n - 1].rows_done[c] == (last if last > first else 0)
        banded_bins += nb.value
    assert banded_bins == bins
    got = frame_of(d)
    for c in range(d.ncomp):
        assert np.array_equal(got[c], oracle_frame[c])


DAMAGED = {}


def damaged_case(size):
    """the image, its one segment and the oracle's stream, once per size"""
    if size not in DAMAGED:
        from lepton_amd import corpus

        img = JpegImage(corpus.synth_jpeg(size[0], size[1], 77))
        segs = img.plan()
        streams, _ = ob.oracle_encode(img.desc, segs)
        DAMAGED[size] = (img, segs[0], streams[0])
    return DAMAGED[size]


def damaged_stream(stream, seed):
    rng = np.random.default_rng(seed)
    n = len(stream)
    p = int(rng.integers(n // 4, 3 * n // 4))
    b = bytearray(stream)
    for i in range(8):
        b[p + i] = int(rng.integers(0, 256))
    return bytes(b)


def oracle_on_damaged(d, s, data):
    """(exit code, frame) of the oracle's decoder on a FILL-ed frame"""
    fill_frame(d)
    im = ob.to_lor(d)
    buf = C.create_string_buffer(data, len(data))
    rc = ob.oracle().lor_decode_segment(C.byref(im), s.luma_y_start, s.luma_y_end, s.is_last, buf, len(data), None)
    return rc, frame_of(d)


def check_failing_block(d, s, oracle_rc, oracle_frame, last, got):
    """what the issue asks of one damaged stream: `last` = the final progress record, `got` = the banded decoder's frame"""
    assert (last.status if last.status >= 0 else None) == oracle_rc
    if oracle_rc == 0:
        assert last.fail_component == last.fail_y == last.fail_x == -1
        for c in range(d.ncomp):
            assert np.array_equal(got[c], oracle_frame[c])
        return
    fc, fy, fx = last.fail_component, last.fail_y, last.fail_x
    assert 0 <= fc < d.ncomp and 0 <= fy < d.height_blocks[fc] and 0 <= fx < d.width_blocks[fc]
    assert last.rows_done[fc] == fy or (last.rows_done[fc] == 0 and fy == segment_rows(d, s, fc)[0])
    for c in range(d.ncomp):
        differ = np.argwhere((got[c] != oracle_frame[c]).any(axis=2))
        assert [tuple(x) for x in differ] == ([(fy, fx)] if c == fc else []), (c, differ[:4], (fc, fy, fx))
        first = segment_rows(d, s, c)[0]
        behind = max(last.rows_done[c], first) + (1 if c == fc else 0)   # rows behind the failing block in schedule order
        for f in (got, oracle_frame):
            assert (f[c][behind:] == FILL).all()
            if c == fc:
                assert (f[c][fy, fx + 1:] == FILL).all()
    assert (got[fc][fy, fx] == FILL).all()   # the failing block itself is not stored


@pytest.mark.parametrize("size", [(96, 64), (203, 149)])
def test_failing_block(emu, size):
    img, s, stream = damaged_case(size)
    d = img.desc
    refused = 0
    for seed in range(40):
        data = damaged_stream(stream, seed)
        oracle_rc, oracle_frame = oracle_on_damaged(d, s, data)
        refused += oracle_rc != 0
        for band in (1, 0):
            fill_frame(d)
            cap = segment_mcu_rows(d, s) + 2
            prog = (abi.DecodeProgress * cap)()
            n = emu.emu_decode_segment_v4_rows(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, data, len(data), band, prog, cap, None)
            assert n >= 1, (seed, band, n)
            check_failing_block(d, s, oracle_rc, oracle_frame, prog[n - 1], frame_of(d))
    assert refused >= 30, refused
