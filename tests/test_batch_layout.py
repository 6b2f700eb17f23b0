"""The batch pipelines' layout rules and launch order -- lepton_amd/csrc/lep_batch_layout.h, the host code that lep_batch.hip reserves,
fills, uploads and launches by -- on numbers made up here (tests/emu/batch_layout_probe.cc): no file is parsed, no GPU is needed.
Every expected number below is worked out by hand from the rules, none is taken from the header."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST, SEQ, PROG = 0, 1, 2    # lepbatch::Route


@pytest.fixture(scope="module")
def probe():
    src, so = os.path.join(ROOT, "tests", "emu", "batch_layout_probe.cc"), os.path.join(ROOT, "tests", "emu", "libbatch_layout_probe.so")
    tmp = "%s.%d" % (so, os.getpid())
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, src])
    os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.emu_scan_arena.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.emu_restart_table_bytes.argtypes = [C.c_uint64]
    lib.emu_restart_table_bytes.restype = C.c_uint64
    lib.emu_stream_slot_bytes.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_int]
    lib.emu_stream_slot_bytes.restype = C.c_uint64
    lib.emu_download_whole.argtypes = [C.c_uint64, C.c_uint64]
    lib.emu_recode_slots.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    lib.emu_verify_arena.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.emu_gpu_answer_stands.argtypes = [C.c_void_p] * 5 + [C.c_int]
    lib.emu_launch_order.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.emu_point_components.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    return lib


def _u32(v):
    return (C.c_uint32 * len(v))(*v)


def _scan_arena(probe, images, verify):
    """images: dicts of route, scan_len, restarts, mcuv, ref_len, prow_need, scans = [(scan_len, restarts, ref_len)]"""
    flat = []
    for im in images:
        scans = im.get("scans", [])
        flat += [im["route"], im.get("scan_len", 0), im.get("restarts", 0), im.get("mcuv", 0), im.get("ref_len", 0), im.get("prow_need", 0), len(scans)]
        for sc in scans:
            flat += list(sc)
    out = (C.c_int64 * (len(flat) + 2))()
    m = probe.emu_scan_arena((C.c_int64 * len(flat))(*flat), len(images), int(verify), out)
    got, p = [], 0
    for im in images:
        ns = len(im.get("scans", []))
        d = dict(zip(("scan_off", "table_off", "ref_off", "row_off"), out[p:p + 4]))
        d["scans"] = [tuple(out[p + 4 + 3 * q: p + 7 + 3 * q]) for q in range(ns)]
        got.append(d)
        p += 4 + 3 * ns
    assert m == p + 2
    return got, out[p], out[p + 1]


FOUR = [dict(route=SEQ, scan_len=1000, mcuv=10, ref_len=1100),                                      # A
        dict(route=PROG, prow_need=25, scans=[(100, 0, 120), (37, 3, 41)]),                         # B
        dict(route=SEQ, scan_len=4097, restarts=20, mcuv=7, ref_len=5000),                          # C
        dict(route=HOST)]                                                                           # D


def test_scan_arena_with_verify(probe):
    (a, b, c, d), scan_total, rows_total = _scan_arena(probe, FOUR, True)
    # rooms: sequential (len + 64) up to 16, progressive (len + 80) up to 16
    assert a["scan_off"] == 0                                   # room 1072 = 1064 -> 1072
    assert c["scan_off"] == 1072 and c["table_off"] == 1072 + 4176 == 5248         # room 4161 -> 4176; 20 positions = 80 bytes
    assert b["scans"][0][0] == 5328                             # 5248 + 80; room 180 -> 192
    assert b["scans"][1][0] == 5520 and b["scans"][1][1] == 5648                   # room 117 -> 128; 3 positions = 12 -> 16 bytes
    assert (b["scans"][0][2], b["scans"][1][2]) == (5664, 5792)                     # 120 -> 128, 41 -> 48
    assert a["ref_off"] == 5840 and c["ref_off"] == 6944        # 1100 -> 1104, 5000 -> 5008
    assert scan_total == 11952
    assert (a["row_off"], c["row_off"], b["row_off"], rows_total) == (0, 11, 19, 44)    # 11 + 8 + 25
    assert d == dict(scan_off=0, table_off=0, ref_off=0, row_off=0, scans=[])


def test_scan_arena_without_verify(probe):
    (a, b, c, d), scan_total, rows_total = _scan_arena(probe, FOUR, False)
    assert scan_total == 5664 and rows_total == 44
    assert (a["scan_off"], c["scan_off"], c["table_off"]) == (0, 1072, 5248)
    assert [s[:2] for s in b["scans"]] == [(5328, 5520), (5520, 5648)]              # (scan, table): scan 0 has no table, 0 bytes at 5520
    assert a["ref_off"] == c["ref_off"] == 0 and [s[2] for s in b["scans"]] == [0, 0]   # no reference offsets


def test_scan_arena_sequential_without_a_reference(probe):
    """under verify an image whose scan has no single file range (ref_len 0) gets no reference copy"""
    got, scan_total, _ = _scan_arena(probe, [dict(route=SEQ, scan_len=16, mcuv=1), dict(route=SEQ, scan_len=16, mcuv=1, ref_len=5)], True)
    assert [g["scan_off"] for g in got] == [0, 80] and got[1]["ref_off"] == 160 and scan_total == 176


def test_restart_table_bytes(probe):
    assert [probe.emu_restart_table_bytes(n) for n in (0, 1, 3, 4, 5, 20)] == [0, 16, 16, 16, 32, 80]


def test_stream_slots(probe):
    assert probe.emu_stream_slot_bytes(100000, 0, 1, 0) == 190720         # 125000 + 65536 = 190536 -> 745 x 256
    assert probe.emu_stream_slot_bytes(100000, 1200, 4, 0) == 190720      # a baseline file never takes the per-block term
    assert probe.emu_stream_slot_bytes(100000, 1200, 4, 1) == 190720      # 1200 x 40 / 4 = 12000 < 125000
    assert probe.emu_stream_slot_bytes(1000, 1200, 4, 1) == 77568         # 12000 > 1250: 77536 -> 303 x 256


def _recode(probe, caps):
    out = (C.c_uint64 * (3 * len(caps) + 1))()
    probe.emu_recode_slots(_u32(caps), len(caps), out)
    return [out[3 * q] for q in range(len(caps))], [out[3 * q + 1] for q in range(len(caps))], [out[3 * q + 2] for q in range(len(caps))], out[3 * len(caps)]


def test_decompress_scan_arena(probe):
    offs, slots, bounds, total = _recode(probe, [50000, 10000, 10000])
    assert slots == [38192, 10000, 10000]              # min(50000, 50000 - 20000 + 8192)
    assert offs == [0, 38192, 48192] and total == 58192    # all three multiples of 16
    assert bounds == [50000, 10000, 10000]
    _, slots, bounds, _ = _recode(probe, [5000, 10000])
    assert slots == [5000, 10000] and bounds == [5000, 10000]   # min(5000, 0 + 8192)


def test_verify_output_arena(probe):
    out = (C.c_uint64 * 8)()
    probe.emu_verify_arena(_u32([4096, 100]), _u32([120, 41]), _u32([10, 0]), 2, out)
    assert (out[0], out[3]) == (184, 100)              # min(4096, 120 + 64), min(100, 41 + 64)
    assert (out[1], out[4], out[6]) == (0, 192, 304)   # 184 -> 192, 100 -> 112
    assert (out[2], out[5], out[7]) == (0, 10, 10)     # correction words


def _stands(probe, slens, pad=(0, 0, 0), attempted=(0, 0, 0)):
    return bool(probe.emu_gpu_answer_stands(_u32(slens), _u32([38192, 10000, 10000]), _u32([50000, 10000, 10000]), _u32(pad), _u32(attempted), 3))


def test_gpu_answer_stands(probe):
    assert not _stands(probe, [38192, 5, 5])           # segment 0 filled a slot smaller than its bound
    assert _stands(probe, [38191, 5, 5])
    assert _stands(probe, [5, 10000, 5])               # slot equals bound: a full slot is the segment's own limit
    for q in range(3):
        assert not _stands(probe, [5, 5, 5], pad=[2 if k == q else 0 for k in range(3)])
    for q in range(2):
        assert not _stands(probe, [5, 5, 5], pad=[1 if k == q else 0 for k in range(3)], attempted=[50000, 10000, 10000])
    assert _stands(probe, [5, 5, 5], pad=[0, 0, 1], attempted=[0, 0, 10000])
    assert not _stands(probe, [5, 5, 5], pad=[0, 0, 1], attempted=[0, 0, 9999])


def test_download_whole(probe):
    assert probe.emu_download_whole(4194304, 1048576) == 1      # 3 x 1 MiB + 1 MiB: equality counts
    assert probe.emu_download_whole(4194304, 1048575) == 0


RAGGED, EVEN = (100, 151, 7000), (100, 150, 6144)     # hi x 2 > lo x 3; exactly 1.5x and exactly the segments that fill the chip
A, B = 0, 1


def _order(probe, chunks, dec_overlap=-1, scan_separate=False, whole_call=False):
    flat = [v for c in chunks for v in c]
    out = (C.c_int32 * (6 * len(chunks)))()
    probe.emu_launch_order((C.c_int64 * len(flat))(*flat), len(chunks), dec_overlap, int(scan_separate), int(whole_call), out)
    return [dict(zip(("stream", "set", "beside", "ragged", "company", "prev_slot"), out[6 * k: 6 * k + 6])) for k in range(len(chunks))]


def test_launch_order_automatic(probe):
    got = _order(probe, [RAGGED, EVEN, RAGGED, EVEN])
    assert [(g["stream"], g["set"], g["beside"]) for g in got] == [(A, 0, 0), (B, 1, 1), (B, 1, 0), (A, 0, 1)]
    assert [g["ragged"] for g in got] == [1, 0, 1, 0]
    assert [g["company"] for g in got] == [1, 1, 1, 1]            # beside || ragged, each
    assert [g["prev_slot"] for g in got] == [-1, 0, 1, 0]
    # few segments are ragged whatever their sizes; an even chunk behind an even chunk is alone in every sense
    got = _order(probe, [(100, 100, 6143), EVEN, EVEN])
    assert [g["ragged"] for g in got] == [1, 0, 0] and [g["beside"] for g in got] == [0, 1, 0] and [g["company"] for g in got] == [1, 1, 0]
    # a chunk that is the whole call has no neighbour
    assert _order(probe, [RAGGED], whole_call=True)[0]["company"] == 0


def test_launch_order_separate_scan_stream(probe):
    for overlap in (-1, 0, 1):
        got = _order(probe, [RAGGED, EVEN, RAGGED, EVEN], dec_overlap=overlap, scan_separate=True)
        assert all((g["stream"], g["set"], g["beside"], g["company"]) == (A, 0, 0, 0) for g in got)


def test_launch_order_forced(probe):
    assert [(g["stream"], g["set"], g["beside"], g["company"]) for g in _order(probe, [RAGGED, EVEN, EVEN], 0)] == [(A, 0, 0, 0)] * 3
    assert [(g["stream"], g["set"], g["beside"], g["company"]) for g in _order(probe, [EVEN, EVEN, EVEN], 1)] == [(A, 0, 0, 0), (B, 1, 1, 1), (A, 0, 1, 1)]


def test_point_components(probe):
    out = (C.c_int64 * 4)()
    probe.emu_point_components(3, _u32([600, 150, 150, 9]), out)
    assert list(out) == [0, 600 * 128, 750 * 128, -1]             # 128 bytes per block; the fourth pointer is null
    probe.emu_point_components(1, _u32([7, 7, 7, 7]), out)
    assert list(out) == [0, -1, -1, -1]
