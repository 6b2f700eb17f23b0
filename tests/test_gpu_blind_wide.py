"""Interleaved scans whose blocks all use one DC and one AC table and whose MCU has more than four blocks (4:2:0 with one pair of tables
is six), on the lane-per-subsequence scan kernels of the HIP build (lep_huffdec_simt.h simt_blind_phases; tests/test_blind_wide_emulation.py
steps the same code on the CPU).  Before, such a scan ended with status 3 after three wasted settle passes and the batch compressor gave it
a second chance with the single-wave kernel; now the lanes settle it, and lep_batch_scan_second_chances() says so."""
import ctypes as C
import os
import sys
import zlib

import numpy as np
import pytest

from lepton_amd import abi
from lepton_amd.codec import GpuCodec, LeptonError

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

WIDE = ["5_y22_c", "6_420", "6_y21_cb21_cr21", "8_y22_cb21_cr21", "10_y22_cb22_cr21", "12_y22_cb22_cr22"]
NARROW = ["3_444", "4_y21_c_c"]
TWO = [(1, 1, 1, 0, 1, 1), (2, 1, 1, 0, 1, 1)]          # two blocks per MCU, tables 1 / 1


def _files(layouts, sizes, density=0.1):
    import jpeg_writer as jw
    from test_blind_wide_emulation import LAYOUTS

    out = []
    for name in layouts:
        comps = TWO if name == "2_two" else LAYOUTS[name]
        for w, h in sizes:
            out.append(("%s %dx%d" % (name, w, h), jw.write_baseline(w, h, comps, np.random.default_rng(zlib.crc32(("%s %d" % (name, w)).encode())), density=density)[0]))
    return out


def _eligible(files, must):
    """the files lep_jpeg_open_gpu takes; a layout in `must` that it does not take fails the test"""
    from test_blind_wide_emulation import _open

    kept = []
    for name, jpg in files:
        one = _open(jpg)
        if one is None:
            assert name.split()[0] not in must, (name, "must be eligible for the GPU scan decoder")
            continue
        abi.lib().lep_jpeg_close(one[3])
        kept.append((name, jpg))
    return kept


def _decode_on_device(codec, jpgs, simt):
    """lep_gpu_huffman_decode_simt_device / lep_gpu_huffman_decode_device on device-resident scans: (row records per file, planes per file)"""
    from test_blind_wide_emulation import _open

    L = abi.lib()
    g = codec.handle

    def dmalloc(n):
        p = C.c_void_p()
        assert L.lep_gpu_malloc(g, n, C.byref(p)) == 0
        return p

    def opened_as_flagged(jpg):     # (a file flagged LEP_HUFFDEC_RST_TABLE: the marker positions go behind its scan bytes, as the flag promises)
        one = _open(jpg)
        if not one[0].flags & 2:
            return one
        L.lep_jpeg_close(one[3])
        return _open(jpg, with_restart_table=True)

    opened = [opened_as_flagged(j) for j in jpgs]
    imgs = (abi.HuffDecImage * len(jpgs))()
    dev, planes_dev, nrows = [], [], []
    rows_total = 0
    for k, (img, scan, planes, h) in enumerate(opened):
        L.lep_jpeg_close(h)
        n = len(scan.raw)
        dscan = dmalloc(n)
        assert L.lep_gpu_memcpy_h2d(g, dscan, scan, n) == 0
        dev.append(dscan)
        C.memmove(C.byref(imgs[k]), C.byref(img), C.sizeof(abi.HuffDecImage))
        imgs[k].scan = dscan.value
        mine = []
        for c in range(img.ncomp):
            nb = len(planes[c].raw)
            p = dmalloc(nb)
            assert L.lep_gpu_memset(g, p, 0, nb) == 0
            dev.append(p)
            mine.append((p, nb))
            imgs[k].blocks[c] = p.value
        planes_dev.append(mine)
        imgs[k].rows_off = rows_total
        nrows.append((rows_total, img.mcuv + 1))
        rows_total += img.mcuv + 1
    nrow_bytes = rows_total * C.sizeof(abi.HuffDecRow)
    drows = dmalloc(nrow_bytes)
    assert L.lep_gpu_memset(g, drows, 0, nrow_bytes) == 0
    fn = L.lep_gpu_huffman_decode_simt_device if simt else L.lep_gpu_huffman_decode_device
    assert fn(g, imgs, len(jpgs), drows, None) == 0
    assert L.lep_gpu_sync(g) == 0
    rows = (abi.HuffDecRow * rows_total)()
    assert L.lep_gpu_memcpy_d2h(g, rows, drows, nrow_bytes) == 0
    records, frames = [], []
    for k in range(len(jpgs)):
        first, n = nrows[k]
        records.append([(rows[first + r].bitpos, tuple(rows[first + r].last_dc), rows[first + r].aux) for r in range(n)])
        mine = []
        for p, nb in planes_dev[k]:
            buf = C.create_string_buffer(nb)
            assert L.lep_gpu_memcpy_d2h(g, buf, p, nb) == 0
            mine.append(buf.raw)
        frames.append(mine)
    for p in dev + [drows]:
        L.lep_gpu_free(g, p)
    return records, frames


def _lane_kernels_equal_the_single_wave_kernel(files):
    codec = GpuCodec(0)        # (LEP_HUFFDEC_SIMT_BITS is read when the codec object is made)
    try:
        jpgs = [j for _, j in files]
        rec1, frm1 = _decode_on_device(codec, jpgs, simt=False)
        rec2, frm2 = _decode_on_device(codec, jpgs, simt=True)
    finally:
        codec.close()
    for k, (name, _) in enumerate(files):
        assert rec1[k][-1][2] >> 8 == 0, (name, "the single-wave kernel reports an irregular scan")
        assert (rec2[k][-1][2] >> 8) & 0x3fffff == 0, (name, "status", (rec2[k][-1][2] >> 8) & 0x3fffff)
        assert frm2[k] == frm1[k], (name, "frames differ")
        assert rec2[k] == rec1[k], (name, "records differ")


def test_gpu_lane_kernels_on_wide_blind_scans_with_short_subsequences(monkeypatch):
    """1024-bit subsequences (hundreds of lanes per file, prefix sums across 64-lane groups, every lane starting in mid-MCU): status 0,
    frame and records of the single-wave kernel"""
    monkeypatch.setenv("LEP_HUFFDEC_SIMT_BITS", "1024")
    files = _eligible(_files(WIDE, [(640, 480), (333, 250)]), must=("5_y22_c", "6_420", "6_y21_cb21_cr21"))
    assert len(files) >= 6
    _lane_kernels_equal_the_single_wave_kernel(files)


def test_gpu_lane_kernels_on_wide_blind_scans_with_the_products_subsequences(monkeypatch):
    """the subsequence length the launch code chooses by itself, at 1920 x 1080"""
    monkeypatch.delenv("LEP_HUFFDEC_SIMT_BITS", raising=False)
    files = _eligible(_files(WIDE, [(1920, 1080)]), must=("5_y22_c", "6_420", "6_y21_cb21_cr21"))
    assert len(files) >= 3
    _lane_kernels_equal_the_single_wave_kernel(files)


@pytest.mark.parametrize("bits", [1024, 0], ids=["1024_bits", "the_rule"])
def test_gpu_lane_kernels_on_a_mixed_launch(monkeypatch, bits):
    """ONE launch of the lane decoder holding wide blind, plain and interval images in this order: six-block 4:2:0, 4:4:4, a 4:2:0 file
    with a restart interval of one MCU row (flagged LEP_HUFFDEC_RST_TABLE: lane = interval), five-block, two-block.  At 1024 bits both
    wide files have more than 64 subsequences (142 and 115), so the launch plan (lep_huffdec_simt.h simt_dec_plan) puts wide wavefronts
    and slot offsets of two wide images on both sides of plain ones; then the subsequence length the plan chooses by itself.  For every
    file: status 0, records and frame of the single-wave kernel."""
    import jpeg_writer as jw
    from test_blind_wide_emulation import _open

    if bits:
        monkeypatch.setenv("LEP_HUFFDEC_SIMT_BITS", str(bits))
    else:
        monkeypatch.delenv("LEP_HUFFDEC_SIMT_BITS", raising=False)
    c420 = [(1, 2, 2, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)]
    interval = ("420 rst 333x250", jw.write_baseline(333, 250, c420, np.random.default_rng(5), density=0.1, restart_interval=21)[0])
    files = _files(["6_420"], [(333, 250)]) + _files(["3_444"], [(97, 50)]) + [interval] + _files(["5_y22_c"], [(333, 250)]) + _files(["2_two"], [(97, 50)])
    assert len(_eligible(files, must=("6_420", "3_444", "420", "5_y22_c", "2_two"))) == 5
    one = _open(interval[1])
    abi.lib().lep_jpeg_close(one[3])
    assert one[0].flags & 2 and one[0].rsti == one[0].mcuh == 21, "the interval file must come flagged: a row of MCUs per interval"
    for k in (0, 3):
        one = _open(files[k][1])
        abi.lib().lep_jpeg_close(one[3])
        assert one[0].scan_len * 8 > 64 * 1024, (files[k][0], "more than one wavefront at 1024 bits")
    _lane_kernels_equal_the_single_wave_kernel(files)


def _flipped(jpg):
    """the file with one byte in the middle of its scan changed (never into a marker's 0xff)"""
    sos = jpg.find(b"\xff\xda")
    at = sos + 14 + (len(jpg) - sos) // 2
    b = bytearray(jpg)
    b[at] ^= 0x55
    if b[at] == 0xFF:
        b[at] = 0x7F
    return bytes(b)


def test_gpu_batch_settles_wide_blind_scans_without_a_second_chance(monkeypatch):
    """compress_batch == the per-file compress, decompress_batch returns the files, every file's Huffman half ran on the GPU, and no scan
    was handed to the single-wave kernel behind the lane decoder.  Control: a six-block file with a byte of its scan flipped -- an
    irregular scan is an ordinary decode status -- is handed on (the counter moves by one) and ends as the per-file path ends it: the
    same .lep, or the reference's refusal."""
    monkeypatch.delenv("LEP_HUFFDEC_SIMT_BITS", raising=False)
    monkeypatch.delenv("LEP_HUFFDEC_SIMT", raising=False)
    files = _eligible(_files(["2_two"] + NARROW + WIDE, [(640, 480), (333, 250), (97, 50)]), must=("2_two", "3_444", "4_y21_c_c", "5_y22_c", "6_420", "6_y21_cb21_cr21"))
    jpgs = [j for _, j in files]
    codec = GpuCodec(0)
    try:
        want = [codec.compress(j) for j in jpgs]
        before = codec.scan_second_chances()
        got, st, cs = codec.compress_batch(jpgs, chunk_images=8)
        assert st == [0] * len(jpgs), st
        assert [files[i][0] for i in range(len(jpgs)) if got[i] != want[i]] == []
        assert cs["gpu_huffman_files"] == len(jpgs), cs
        assert codec.scan_second_chances() - before == 0
        back, st2, ds = codec.decompress_batch(got, chunk_images=8)
        assert st2 == [0] * len(jpgs) and back == jpgs
        assert ds["gpu_huffman_files"] == len(jpgs), ds
        assert codec.scan_second_chances() - before == 0
        # the control
        six = dict(files)["6_420 640x480"]
        bad = _flipped(six)
        rec, _ = _decode_on_device(codec, [bad], simt=True)
        assert (rec[0][-1][2] >> 8) & 0x3fffff != 0, "the flipped byte left a regular scan: no control"
        try:
            per_file = codec.compress(bad)
        except LeptonError:
            per_file = None
        before = codec.scan_second_chances()
        got, st, _ = codec.compress_batch([six, bad], chunk_images=8)
        assert codec.scan_second_chances() - before == 1
        assert st[0] == 0 and got[0] == want[[n for n, _ in files].index("6_420 640x480")]
        if per_file is None:
            assert st[1] != 0 and got[1] is None          # the reference's refusal, through the host parser
        else:
            assert st[1] == 0 and got[1] == per_file
    finally:
        codec.close()
