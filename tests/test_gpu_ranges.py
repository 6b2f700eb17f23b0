"""lep_decompress_batch_ranges / lep_decompress_range on the GPU: part of a restored file from the thread segments it needs.

Equality: every answer is decompress(lep)[first:first + len] -- whole files and a slice, one and three components, a cut file, restart
intervals, a progressive file (the whole-file path) and a four-segment file compressed here, for ranges at every part boundary, at bands
of 1 and 4 MCU rows and the doubling schedule.  Economy, through the call's counters: a range in the head launches nothing, a range inside
one segment begins one segment, the first scan bytes retire their segment after a fraction of its rows, only the window's bytes cross
PCIe, no frame does, and the doubling schedule stays within its bound.  Independence: damage in a segment the range does not touch is
not seen, and files of a batch fail alone.  Sessions: the same requests under LEP_STREAM_SESSION_FILES=2."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import jpeg_writer as jw
from conftest import GOLDEN, golden
from lepton_amd import abi
from lepton_amd.codec import JpegImage, LepFile, LeptonError
from test_decode_rows_emulation import damaged_stream
from test_gpu_stream_batch import environment
from test_range_bands_emulation import plan_of, ranges_of

pytestmark = pytest.mark.gpu

STREAMED = ["c420_odd_203x149", "q30_256x256_4seg", "rst_c420_176x112", "slice_4seg_q97", "gray_120x88", "truncated", "gen_c420_4seg"]
NAMES = STREAMED + ["prog_c420_320x240"]
C420 = [(1, 2, 2, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)]


def generated_jpeg():
    """dense 4:2:0, 560 x 400, ~270 KB: a size that gets four hand-offs"""
    return jw.write_baseline(560, 400, C420, np.random.default_rng(9), density=0.9, amp=300.0, quality=50)[0]


@pytest.fixture(scope="module")
def files(gpu_codec):
    """per file, once: (.lep, what decompress restores, the whole-file range plan)"""
    man = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    out = {}
    for name in NAMES:
        if name.startswith("gen_"):
            jpg = generated_jpeg()
            lep = gpu_codec.compress(jpg)
            want = jpg
        else:
            jpg, lep = golden(name)
            want = jpg[man[name]["slice"][0]:man[name]["slice"][1]] if "slice" in man[name] else jpg
        assert gpu_codec.decompress(lep) == want
        out[name] = (lep, want, plan_of(lep))
    assert out["gen_c420_4seg"][2].nseg == 4 and out["gen_c420_4seg"][2].sizes_known == 1
    assert all(out[n][2].in_session == 1 for n in STREAMED) and out["prog_c420_320x240"][2].in_session == 0
    return out


def cut(want, first, length):
    return want[first:first + length] if length else want[first:]


def segment_rows(lep):
    f = LepFile(lep)
    img, segs = abi.HuffImage(), (abi.HuffSegment * abi.MAX_SEGMENTS)()
    nseg, ok = C.c_int(0), C.c_int(0)
    assert abi.lib().lep_file_recode_plan(f.handle, C.byref(img), segs, C.byref(nseg), C.byref(ok)) == 0 and ok.value
    return [segs[q].mcu_row1 - segs[q].mcu_row0 for q in range(nseg.value)]


@pytest.mark.parametrize("band", [1, 4, 0])
def test_ranges_equal_the_whole_decode(gpu_codec, files, band):
    assert abi.lib().lep_gpu_stream_pack(gpu_codec.handle) == 1
    leps, ranges, wants = [], [], []
    for name in NAMES:
        lep, want, rp0 = files[name]
        if rp0.nseg:
            rs = ranges_of(rp0, seed=band, randoms=4)
        else:
            rs = [(0, 0), (0, 1), (100, 5000), (len(want) - 1, 0), (len(want) - 1, 10), (len(want), 4), (7, len(want))]
        rs += [(len(want), 0), (len(want) + 5, 3)]   # at and behind the end: empty
        for first, length in rs:
            leps.append(lep); ranges.append((first, length)); wants.append(cut(want, first, length))
    outs, status, stats = gpu_codec.decompress_batch_ranges(leps, ranges, band)
    assert status == [0] * len(leps)
    bad = [(r, len(o), len(w)) for o, w, r in zip(outs, wants, ranges) if o != w]
    assert not bad, bad[:5]
    assert stats["frame_bytes_down"] == 0
    assert stats["files_ranged"] + stats["files_whole"] + stats["files_no_decode"] == len(leps)
    n_prog = sum(1 for lep in leps if lep is files["prog_c420_320x240"][0])
    assert stats["files_whole"] == n_prog and stats["files_no_decode"] > 0 and stats["files_ranged"] > 100
    assert stats["segments_begun"] < stats["segments_total"] and stats["segments_retired"] > 0
    assert stats["mcu_rows_decoded"] < stats["mcu_rows_begun"]
    assert stats["writer_launches"] <= stats["advances"]


def test_the_single_file_call(gpu_codec, files):
    for name in ("q30_256x256_4seg", "slice_4seg_q97", "prog_c420_320x240", "gray_120x88"):
        lep, want, rp0 = files[name]
        for first, length in ((0, 0), (0, 700), (len(want) // 2, 4096), (len(want) - 3, 0), (len(want), 0), (len(want) + 1, 9)):
            assert gpu_codec.decompress_range(lep, first, length) == cut(want, first, length), (name, first, length)
    with pytest.raises(LeptonError) as e:
        gpu_codec.decompress_range(b"\xcf\x84" + bytes(40), 0, 10)
    with pytest.raises(LeptonError) as whole:
        gpu_codec.decompress(b"\xcf\x84" + bytes(40))
    assert e.value.code == whole.value.code


def test_economy(gpu_codec, files):
    assert abi.lib().lep_gpu_stream_pack(gpu_codec.handle) == 1   # (only the packed path moves windows alone)
    lep, want, rp = files["gen_c420_4seg"]
    rows = segment_rows(lep)
    # a range in the head: nothing is begun, nothing is launched
    outs, status, st = gpu_codec.decompress_batch_ranges([lep], [(2, rp.head_len - 2)], 1)
    assert status == [0] and outs[0] == want[2:rp.head_len]
    assert (st["segments_begun"], st["advances"], st["sessions"], st["writer_launches"], st["files_no_decode"], st["scan_bytes_down"]) == (0, 0, 0, 0, 1, 0)
    # a range inside segment 1 or 2: one segment is begun, and only the window's bytes come down
    for q in (1, 2):
        first, length = rp.seg_first[q] + rp.seg_len[q] // 3, 3001
        outs, status, st = gpu_codec.decompress_batch_ranges([lep], [(first, length)], 4)
        assert status == [0] and outs[0] == want[first:first + length]
        assert (st["segments_begun"], st["segments_total"], st["sessions"], st["files_ranged"]) == (1, 4, 1, 1)
        assert st["scan_bytes_down"] == length and st["frame_bytes_down"] == 0
        assert st["segments_retired"] == 1 and st["mcu_rows_begun"] == rows[q] and 0 < st["mcu_rows_decoded"] < rows[q]
    # the first 512 bytes of the scan at band 1: segment 0 is retired after a fraction of its rows
    outs, status, st = gpu_codec.decompress_batch_ranges([lep], [(rp.head_len, 512)], 1)
    assert status == [0] and outs[0] == want[rp.head_len:rp.head_len + 512]
    assert st["segments_retired"] == 1 and st["segments_begun"] == 1 and st["mcu_rows_decoded"] < st["mcu_rows_begun"] == rows[0]
    assert st["scan_bytes_down"] == 512 and st["advances"] < rows[0]
    # scan bytes down = the requested bytes that lie in segment extents: across head / segment 0, across segments 1 / 2, into the tail
    tail0 = rp.jpeg_size - rp.tail_len
    for first, length, in_segments in ((rp.head_len - 100, 300, 200), (rp.seg_first[2] - 1000, 2500, 2500), (tail0 - 50, 0, 50), (tail0, 0, 0)):
        outs, status, st = gpu_codec.decompress_batch_ranges([lep], [(first, length)], 0)
        assert status == [0] and outs[0] == cut(want, first, length)
        assert st["scan_bytes_down"] == in_segments and st["frame_bytes_down"] == 0, (first, length)
    # the doubling schedule: at most ceil(log2 rows) + 1 advances for the rows of the longest touched segment
    for first, length in ((rp.head_len, 512), (rp.seg_first[1] + 5, 0), (0, 0), (rp.seg_first[3] - 1, 2)):
        r = plan_of(lep, first, length)
        longest = max(rows[r.first_seg:r.last_seg + 1])
        outs, status, st = gpu_codec.decompress_batch_ranges([lep], [(first, length)], 0)
        assert status == [0] and outs[0] == cut(want, first, length)
        assert 1 <= st["advances"] <= (longest - 1).bit_length() + 1, (first, length, st["advances"], longest)


def test_no_frame_comes_down_for_any_streamed_fixture(gpu_codec, files):
    leps = [files[n][0] for n in STREAMED]
    ranges = [(files[n][2].head_len + 1, 777) for n in STREAMED]
    outs, status, st = gpu_codec.decompress_batch_ranges(leps, ranges, 0)
    assert status == [0] * len(leps) and st["frame_bytes_down"] == 0 and st["files_ranged"] == len(leps) and st["files_whole"] == 0
    assert outs == [cut(files[n][1], *r) for n, r in zip(STREAMED, ranges)]
    assert st["scan_bytes_down"] == sum(len(o) for o in outs)


@pytest.fixture(scope="module")
def damaged(gpu_codec, files):
    """the four-segment file with segment 2's stream damaged in its middle: (.lep, what lep_decompress says about it)"""
    img = JpegImage(generated_jpeg())
    segs = img.plan()
    streams = gpu_codec.encode([img], [segs])[0]
    assert len(streams) == 4 and img.write_lep(streams) == files["gen_c420_4seg"][0]
    for seed in range(8):
        bad = list(streams)
        bad[2] = damaged_stream(streams[2], seed)
        lep = img.write_lep(bad)
        try:
            whole = gpu_codec.decompress(lep)
        except LeptonError as e:
            return lep, e.code
        if whole != files["gen_c420_4seg"][1]:
            return lep, 0
    raise AssertionError("no seed damaged the file")


def test_damage_outside_the_range_is_not_seen(gpu_codec, files, damaged):
    good, want, rp = files["gen_c420_4seg"]
    lep, code = damaged
    r0 = (rp.seg_first[0] + 100, 5000)
    outs, status, st = gpu_codec.decompress_batch_ranges([lep], [r0], 1)
    assert status == [0] and outs[0] == cut(want, *r0) and st["segments_begun"] == 1
    assert gpu_codec.decompress_range(lep, rp.seg_first[3] + 10, 2000) == cut(want, rp.seg_first[3] + 10, 2000)   # ... nor behind it
    if code:   # a range that touches the damaged segment gets the decode's code
        outs, status, st = gpu_codec.decompress_batch_ranges([lep], [(rp.seg_first[2] + 10, 0)], 4)
        assert status == [code] and outs == [None]
    # a mixed batch: every neighbour is untouched, the file that does not parse gets lep_decompress's code
    prog, prog_want, _ = files["prog_c420_320x240"]
    junk = b"\xcf\x84" + bytes(40)
    with pytest.raises(LeptonError) as e:
        gpu_codec.decompress(junk)
    leps = [good, lep, prog, junk, good, lep, lep]
    ranges = [(0, 0), r0, (1000, 9000), (0, 10), (rp.seg_first[1] - 10, 50000), (rp.seg_first[2] - 500, rp.seg_len[2] + 600), (rp.seg_first[2] - 500, 1000)]
    outs, status, st = gpu_codec.decompress_batch_ranges(leps, ranges, 4)
    assert status[:5] == [0, 0, 0, e.value.code, 0]
    assert outs[0] == want and outs[1] == cut(want, *r0) and outs[2] == cut(prog_want, 1000, 9000) and outs[3] is None
    assert outs[4] == cut(want, *ranges[4])
    if code:   # through the damaged segment: the decode's code.  Into its first bytes, in front of the damage: retired before the decoder gets there
        assert status[5] == code and outs[5] is None
    assert status[6] == 0 and outs[6] == cut(want, *ranges[6])
    assert st["files_whole"] == 2 and st["files_ranged"] == 5


def test_sessions_of_two_files(gpu_codec, files):
    names = ["gen_c420_4seg", "q30_256x256_4seg", "gray_120x88", "gen_c420_4seg", "slice_4seg_q97", "truncated", "prog_c420_320x240"]
    leps = [files[n][0] for n in names]
    ranges = [(files[n][2].head_len + 7 * i, 20000 + i) for i, n in enumerate(names)]
    with environment(LEP_STREAM_SESSION_FILES="2"):
        from lepton_amd.codec import GpuCodec

        codec = GpuCodec(0)
        try:
            outs, status, st = codec.decompress_batch_ranges(leps, ranges, 4)
        finally:
            codec.close()
    assert status == [0] * len(names)
    assert outs == [cut(files[n][1], *r) for n, r in zip(names, ranges)]
    assert st["files_ranged"] == 6 and st["sessions"] == 3 and st["files_whole"] == 1 and st["frame_bytes_down"] == 0
