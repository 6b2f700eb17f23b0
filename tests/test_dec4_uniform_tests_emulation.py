"""The v4 decoder with its wave-uniform tests held as scalars, its lane-range tests written as selects and the update's second regrouped
pass (lep_dec4.h LEP_DEC4_UNIFORM_TESTS / LEP_DEC4_LANE_SELECTS / LEP_DEC4_WORD_PER_LANE_2), stepped on the CPU through
tests/emu/dec4_uniform_emu.cc: whole segments, cut streams and the resumable form against the oracle, in the shipped assignment of the
serial rounds, with -DLEP_DEC4_SCALAR=13, and with each switch at 0 (the A/B builds).  The lane-loop emulation cannot see exec masks -- tests/test_gpu_dec4_uniform_tests.py is the one that catches a wrong
select on the hardware; this one holds the source-level rewrite: clamped indices, hoisted branches, the neighbour cases.

The shapes are the smallest that meet every arm the change touches: one block (neither neighbour), one row of blocks (left neighbours
only), one column (above only), one 4:2:0 MCU (chroma: neither; luma: all four cases), ragged edges with enough blocks for counts to
wrap, and coefficients of |v| >= 8 in the interior, at the edges and in the DC."""
import ctypes as C
import io
import os
import subprocess

import pytest

from conftest import ROOT, golden
from lepton_amd import abi, corpus
from lepton_amd.codec import JpegImage
import oracle_binding as ob
import test_dec4_word_per_lane_emulation as wpl
from test_dec4_word_per_lane_emulation import cut_case, cut_lengths, fill_frame, frame_of, oracle_on, same_frame_up_to_the_refused_block

# name: (flags, knobs bits 0..5 expected: uniform tests, lane selects, word per lane, refill groups, second pass asked for / in force)
BUILDS = {
    "shipped": ([], 0b111111),
    "scalar13": (["-DLEP_DEC4_SCALAR=13"], 0b111111),
    "uniform_tests_0": (["-DLEP_DEC4_UNIFORM_TESTS=0"], 0b111110),
    "lane_selects_0": (["-DLEP_DEC4_LANE_SELECTS=0"], 0b011101),   # the second pass is written on the branch-free maps: off with them
    "word_per_lane_2_0": (["-DLEP_DEC4_WORD_PER_LANE_2=0"], 0b001111),
    "all_0": (["-DLEP_DEC4_UNIFORM_TESTS=0", "-DLEP_DEC4_LANE_SELECTS=0", "-DLEP_DEC4_WORD_PER_LANE_2=0"], 0b001100),
}


def _build(name, flags):
    src = os.path.join(ROOT, "tests", "emu", "dec4_uniform_emu.cc")
    so = os.path.join(ROOT, "tests", "emu", "libcore_emu_dec4uni_%s.so" % name)
    tmp = "%s.%d" % (so, os.getpid())
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared"] + flags + ["-o", tmp, src])
    os.replace(tmp, so)
    L = C.CDLL(so)
    L.emu_decode_segment_v4_rows.argtypes = [C.POINTER(abi.ImageDesc), C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_uint32, C.c_int,
                                             C.POINTER(abi.DecodeProgress), C.c_int, C.POINTER(C.c_uint32)]
    return L


@pytest.fixture(scope="module", params=sorted(BUILDS))
def emu(request):
    flags, want = BUILDS[request.param]
    L = _build(request.param, flags)
    knobs = L.emu_dec4_uniform_knobs()
    assert knobs & 63 == want, "the emulation was not built in the form asked for"
    assert knobs >> 8 == (13 if request.param == "scalar13" else 2)
    return L


def gray_of(jpg):
    """the picture of a corpus.synth_jpeg file as a one-component baseline JPEG"""
    from PIL import Image

    buf = io.BytesIO()
    Image.open(io.BytesIO(jpg)).convert("L").save(buf, format="JPEG", quality=90, optimize=False)
    return buf.getvalue()


def _images():
    out = {}
    for name in ("one_block_8x8", "c420_odd_203x149", "gray_120x88"):
        out[name] = lambda name=name: JpegImage(golden(name)[0])
    out["one_row_64x8_gray"] = lambda: JpegImage(gray_of(corpus.synth_jpeg(64, 8, 31)))      # left neighbours only
    out["one_col_8x64_gray"] = lambda: JpegImage(gray_of(corpus.synth_jpeg(8, 64, 32)))      # above neighbours only
    out["one_mcu_16x16_c420"] = lambda: JpegImage(corpus.synth_jpeg(16, 16, 33))             # chroma: neither; luma: all four cases
    out["large_64x48_q100"] = wpl.IMAGES["large_64x48_q100"]
    out["large_dc_64x48"] = wpl.IMAGES["large_dc_64x48"]
    return out


IMAGES = _images()
CASES = {}


def case(name):
    """once per image: (image, segments, oracle streams, oracle bins, frame bytes per component)"""
    if name not in CASES:
        img = IMAGES[name]()
        segs = img.plan()
        streams, bins = ob.oracle_encode(img.desc, segs)
        frame = [C.string_at(img.desc.blocks[c], img.desc.nblocks(c) * 128) for c in range(img.desc.ncomp)]
        CASES[name] = (img, segs, streams, bins, frame)
    return CASES[name]


def test_the_generated_shapes_are_what_they_are_meant_to_be():
    for name, ncomp, blocks in (("one_row_64x8_gray", 1, (8, 1)), ("one_col_8x64_gray", 1, (1, 8)), ("one_mcu_16x16_c420", 3, (2, 2))):
        d = case(name)[0].desc
        assert d.ncomp == ncomp and (d.width_blocks[0], d.height_blocks[0]) == blocks, (name, d.ncomp, d.width_blocks[0], d.height_blocks[0])
    d = case("one_mcu_16x16_c420")[0].desc
    assert (d.width_blocks[1], d.height_blocks[1], d.width_blocks[2], d.height_blocks[2]) == (1, 1, 1, 1)


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_segments_equal_the_oracle(emu, name):
    img, segs, streams, bins, frame = case(name)
    d = img.desc
    fill_frame(d)
    total = 0
    for s, w in zip(segs, streams):
        nb = C.c_uint32(0)
        assert emu.emu_decode_segment_v4(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, w, len(w), C.byref(nb)) == 0
        total += nb.value
    assert total == bins
    for c in range(d.ncomp):
        n = d.coded_blocks[c] * 128
        assert C.string_at(d.blocks[c], n) == frame[c][:n]


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_bands_of_one_mcu_row_give_the_one_shot_frame(emu, name):
    img, segs, streams, bins, frame = case(name)
    d = img.desc
    fill_frame(d)
    total = 0
    for s, w in zip(segs, streams):
        cap = d.mcu_rows + 2
        prog = (abi.DecodeProgress * cap)()
        nb = C.c_uint32(0)
        n = emu.emu_decode_segment_v4_rows(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, w, len(w), 1, prog, cap, C.byref(nb))
        assert n >= 1 and prog[n - 1].status == 0, (n, prog[max(n, 1) - 1].status)
        total += nb.value
    assert total == bins
    for c in range(d.ncomp):
        n = d.coded_blocks[c] * 128
        assert C.string_at(d.blocks[c], n) == frame[c][:n]


@pytest.mark.parametrize("k", [2, 8, 9])   # 2 bytes, 200 bytes, half the stream
def test_cut_streams_end_as_the_oracle_s_do(emu, k):
    img, s, stream = cut_case()
    d = img.desc
    data = stream[:cut_lengths(len(stream))[k]]
    want_rc, want_frame = oracle_on(d, s, data)
    fill_frame(d)
    rc = emu.emu_decode_segment_v4(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, data, len(data), None)
    assert rc == want_rc
    one_shot = frame_of(d)
    same_frame_up_to_the_refused_block(d, rc, one_shot, want_frame)
