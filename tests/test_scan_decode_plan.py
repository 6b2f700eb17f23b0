"""The scan decoders' launch plans -- lep_huffdec_simt.h simt_dec_plan and lep_scan_decode_plan.h prog_dec_plan, the host code that
lep_gpu_huffman_decode_simt_device and lep_gpu_huffman_progressive_decode_device follow and that tests/emu/scan_dec_driver.h steps -- on
descriptors made up here (tests/emu/scan_dec_plan_probe.cc): only geometry, flags, scan_len, rsti, level, band and frame pointer are
looked at, no scan byte is read.  Every expected number below is worked out by hand from the rules, none is taken from the plans."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lepton_amd import abi  # noqa: E402

RST_TABLE = 2            # LEP_HUFFDEC_RST_TABLE
WIN, RST = 1, 2          # lephuff::kProgDecWin, kProgDecRst (ProgDecScan::pad)
MIN_BITS = 8192          # lephuff::kSimtMinBits


@pytest.fixture(scope="module")
def probe():
    src, so = os.path.join(ROOT, "tests", "emu", "scan_dec_plan_probe.cc"), os.path.join(ROOT, "tests", "emu", "libscan_dec_plan_probe.so")
    tmp = "%s.%d" % (so, os.getpid())
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, src])
    os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.emu_simt_dec_plan.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    lib.emu_prog_dec_plan.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    return lib


def _image(scan_len, luma=1, one_table_pair=False, mcuc=50, rsti=0, flags=0, ncomp=3):
    """three components, luma luma x luma blocks per MCU; one_table_pair: every component on tables 0 / 0"""
    im = abi.HuffDecImage()
    im.scan_len, im.ncomp, im.mcuh, im.mcuv, im.mcuc, im.rsti, im.flags = scan_len, ncomp, mcuc, 1, mcuc, rsti, flags
    for c in range(ncomp):
        im.hs[c] = im.vs[c] = luma if c == 0 else 1
        im.scan_cmp[c] = c
        im.dc_tbl[c] = im.ac_tbl[c] = 0 if (c == 0 or one_table_pair) else 1
    return im


def _simt_plan(probe, images, forced, target, want_rc=0):
    arr = (abi.HuffDecImage * len(images))(*images)
    head, per, waves = (C.c_uint64 * 5)(), (C.c_uint32 * (5 * len(images)))(), (C.c_uint32 * 128)()
    rc = probe.emu_simt_dec_plan(arr, len(images), forced, target, head, per, waves, 64)
    assert (rc != 0) == (want_rc != 0), rc
    if rc:
        return None
    imgs = [dict(zip(("first", "nsub", "sub_bits", "changed0", "slots"), per[5 * i: 5 * i + 5])) for i in range(len(images))]
    assert head[4] <= 64
    return dict(nw_plain=head[0], nsub_all=head[1], nslots=head[2], L=head[3], images=imgs, waves=[(waves[2 * w], waves[2 * w + 1]) for w in range(head[4])])


def test_lane_decoder_plan_of_a_mixed_launch(probe):
    """wide blind (six blocks per MCU, one table pair), plain 4:4:4, table-flagged interval image, wide blind, plain; 1000 bits forced"""
    five = [_image(20000, 2, True), _image(1000), _image(3000, 2, mcuc=103, rsti=5, flags=RST_TABLE), _image(9000, 2, True), _image(12800)]
    p = _simt_plan(probe, five, 1000, 64 * 8192 * 2)
    assert p["L"] == 1024                                              # a forced length is rounded up to 32 bits
    assert [i["sub_bits"] for i in p["images"]] == [1024] * 5
    # ceil(160000 / 1024), ceil(8000 / 1024), (103 - 1) // 5 + 1 intervals, ceil(72000 / 1024), 102400 / 1024
    nsub = [157, 8, 21, 71, 100]
    assert [i["nsub"] for i in p["images"]] == nsub
    assert [i["first"] for i in p["images"]] == [0, 157, 165, 186, 257] and p["nsub_all"] == 357      # cumulative in image order
    assert [i["changed0"] for i in p["images"]] == [0, 0, 0xff, 0, 0]
    # plain and interval wavefronts in front of all wide ones, each group in image order, first_sub stepping by 64
    assert p["waves"] == [(1, 0), (2, 0), (4, 0), (4, 64), (0, 0), (0, 64), (0, 128), (3, 0), (3, 64)]
    assert p["nw_plain"] == 4
    assert [i["slots"] for i in p["images"]] == [0, 0, 0, 157, 0] and p["nslots"] == 157 + 71           # only the two wide images, cumulative


def test_lane_decoder_plan_subsequence_rule(probe):
    # a tiny launch: 800 bits over a million lanes; 64 x (800 / 30 blocks) = 1706 bits: the floor of kSimtMinBits holds
    p = _simt_plan(probe, [_image(100, mcuc=10)], 0, 1 << 20)
    assert p["L"] == MIN_BITS and p["images"][0] == dict(first=0, nsub=1, sub_bits=MIN_BITS, changed0=0, slots=0)
    # many large scans: 4 x 32,000,000 bits over 1000 lanes = 128,000 (a multiple of 32); 64 average blocks are 64 x 32e6 / 300,000 = 6826 bits
    big = [_image(4000000, mcuc=100000) for _ in range(4)]
    p = _simt_plan(probe, big, 0, 1000)
    assert p["L"] == 128000 and all(i["sub_bits"] == 128000 and i["nsub"] == 250 for i in p["images"])
    assert [i["first"] for i in p["images"]] == [0, 250, 500, 750]
    # ... and between them one image of 1000 blocks in the same 32,000,000 bits: 64 x 32,000 = 2,048,000 bits, more than the launch's
    # 5 x 32e6 / 1000 = 160,000 -- that image gets the larger value (16 subsequences: ceil(32e6 / 2,048,000)), its neighbours do not
    mixed = big[:2] + [_image(4000000, mcuc=1000, ncomp=1)] + big[2:]
    p = _simt_plan(probe, mixed, 0, 1000)
    assert p["L"] == 160000
    assert [i["sub_bits"] for i in p["images"]] == [160000, 160000, 2048000, 160000, 160000]
    assert [i["nsub"] for i in p["images"]] == [200, 200, 16, 200, 200]


def test_lane_decoder_plan_refusals(probe):
    _simt_plan(probe, [_image(1000), _image(1000, rsti=5)], 0, 1000, want_rc=1)                       # an interval, no marker table
    _simt_plan(probe, [_image(1000, rsti=0, flags=RST_TABLE)], 0, 1000, want_rc=1)                    # the table flag, no interval
    _simt_plan(probe, [_image(1000, rsti=-1, flags=RST_TABLE)], 0, 1000, want_rc=1)
    _simt_plan(probe, [_image(1000, rsti=5, mcuc=0, flags=RST_TABLE)], 0, 1000, want_rc=1)            # ... no MCUs
    # 2 x (2^31 - 1) intervals: more than 0x7fffffff subsequences -- refused in front of the wave list (which would be 2^26 entries)
    huge = [_image(1000, rsti=1, mcuc=0x7fffffff, flags=RST_TABLE) for _ in range(2)]
    _simt_plan(probe, huge, 0, 1000, want_rc=1)
    assert _simt_plan(probe, [_image(1000, rsti=1 << 20, mcuc=0x7fffffff, flags=RST_TABLE)], 0, 1000)["images"][0]["nsub"] == 2048   # (the bound, not the MCU count)


A, B, SEQ = 0x1000, 0x2000, 0x3000      # the three files' frames (never dereferenced)


def _scan(frame, ident, level, band, sah=0, cmpc=1, rsti=0, flags=0, scan_len=500, first_cmp=0):
    s = abi.HuffProgDecScan()
    s.t = _image(scan_len, 2, mcuc=100, rsti=rsti, flags=flags)
    s.t.blocks[0] = frame
    s.t.rows_off = s.result_off = ident
    s.cmpc, s.from_, s.to, s.sah, s.level = cmpc, band[0], band[1], sah, level
    for c in range(4):
        s.cmp[c] = first_cmp + c if c < cmpc else 0
        s.nch[c], s.ncv[c], s.bcv[c] = 20, 10, 10
    return s


def _three_files():
    """file A: progressive, two levels, scans 0 and 3 table-flagged; file B: progressive, three levels, no intervals; the third file: a
    sequential frame in two scans, one with an interval (and no table), one without.  Interleaved; a scan's name is its index."""
    return [_scan(A, 0, 0, (0, 0), cmpc=3, rsti=2, flags=RST_TABLE, scan_len=10000),    # A: DC, 100 MCUs in intervals of 2
            _scan(B, 1, 0, (0, 0), cmpc=3),                                              # B: DC
            _scan(SEQ, 2, 0, (0, 63), rsti=3, scan_len=700),                             # sequential, an interval: the single-wave kernel's
            _scan(A, 3, 1, (1, 5), rsti=2, flags=RST_TABLE, scan_len=4000),              # A: luma 1..5, 20 x 10 blocks in intervals of 2
            _scan(B, 4, 1, (1, 5)),                                                      # B: luma 1..5
            _scan(SEQ, 5, 0, (0, 63), cmpc=2, scan_len=700),                             # sequential, none: the lane decoder's
            _scan(A, 6, 1, (6, 63), scan_len=900),                                       # A: luma 6..63, no interval: the window form's
            _scan(B, 7, 2, (1, 5), sah=1),                                               # B: luma 1..5 refined (follows scan 4)
            _scan(A, 8, 0, (1, 5), rsti=4, scan_len=900, first_cmp=1),                   # A: Cb 1..5, an interval, no table: neither form's mark
            _scan(B, 9, 1, (0, 0), sah=1, cmpc=3)]                                       # B: DC refined (follows scan 1)


def _prog_plan(probe, scans, lanes=1, win=1, rst=1, floor=1024, pipeline=1, pipeline_max=16384, split=0):
    arr = (abi.HuffProgDecScan * len(scans))(*scans)
    knobs = (C.c_int64 * 7)(lanes, win, rst, floor, pipeline, pipeline_max, split)
    out = (C.c_int64 * 4096)()
    n = probe.emu_prog_dec_plan(arr, len(scans), knobs, out, 4096)
    if n < 0:
        return n
    it = iter(out[:n])
    take = lambda k: [next(it) for _ in range(k)]   # noqa: E731
    p = dict(seq_lanes=take(next(it)), seq_single=take(next(it)))
    p["b"] = [tuple(take(3)) for _ in range(next(it))]          # (order, result_off, pad)
    p["cut"] = take(next(it))
    p["pipelined"], p["b_any_win"] = take(2)
    p["deps"] = [take(4) for _ in range(next(it))]
    p["plain"] = [tuple(take(2)) for _ in range(next(it))]      # (result_off, pad)
    p["pcut"] = take(65)
    p["rst"] = [tuple(take(4)) for _ in range(next(it))]        # (result_off, pad, piece0, npieces)
    p["rcut"] = take(65)
    p["pieces"], p["c_any_win"] = take(2)
    assert not list(it)
    return p


def test_progressive_plan_of_three_files(probe):
    p = _prog_plan(probe, _three_files())
    assert p["seq_lanes"] == [5] and p["seq_single"] == [2]
    # file A, all of it and nothing of B: by level, the flagged scans marked for the interval form, the window mark where prog_win_takes
    # holds (no interval), none on the scan with an interval and no table.  Pieces, floor 1024: scan 0 has 50 intervals in 10000 bytes --
    # ceil(1024 * 50 / 10000) = 6 to a piece, 9 pieces; scan 3 has 100 in 4000 -- 26 to a piece, 4 pieces
    assert p["rst"] == [(0, RST, 0, 9), (3, RST, 9, 4)] and p["pieces"] == 13
    assert p["rcut"] == [0, 1] + [2] * 63
    assert p["plain"] == [(8, 0), (6, WIN)] and p["c_any_win"] == 1
    assert p["pcut"] == [0, 1] + [2] * 63
    # file B: stable by level, order = the caller's indices, one pipelined launch
    assert p["b"] == [(1, 1, WIN), (4, 4, WIN), (9, 9, WIN), (7, 7, WIN)] and p["b_any_win"] == 1
    assert p["pipelined"] == 1
    assert p["deps"] == [[-1] * 4, [-1] * 4, [0, -1, -1, -1], [1, -1, -1, -1]]          # (indices into the launch: 9 follows 1, 7 follows 4)


def test_progressive_plan_knob_by_knob(probe):
    scans = _three_files()
    p = _prog_plan(probe, scans, lanes=0)
    assert p["seq_lanes"] == [] and p["seq_single"] == [2, 5]
    p = _prog_plan(probe, scans, win=0)
    assert [x[2] for x in p["b"]] == [0] * 4 and p["plain"] == [(8, 0), (6, 0)] and not p["b_any_win"] and not p["c_any_win"]
    assert [x[1] for x in p["rst"]] == [RST, RST]
    p = _prog_plan(probe, scans, rst=0)                               # the interval form off: A joins the others
    assert p["rst"] == [] and p["plain"] == [] and p["pieces"] == 0
    assert [x[0] for x in p["b"]] == [0, 1, 8, 3, 4, 6, 9, 7]
    assert [x[2] for x in p["b"]] == [0, WIN, 0, 0, WIN, WIN, WIN, WIN]
    assert p["pipelined"] == 1 and p["cut"] == [0, 3, 7, 8]
    p = _prog_plan(probe, scans, floor=1)                             # a piece per interval
    assert p["rst"] == [(0, RST, 0, 50), (3, RST, 50, 100)] and p["pieces"] == 150
    for kw in (dict(pipeline=0), dict(pipeline_max=3)):               # no pipelining: a launch per level
        p = _prog_plan(probe, scans, **kw)
        assert p["pipelined"] == 0 and p["deps"] == [] and p["cut"] == [0, 1, 3, 4], kw
        assert [x[0] for x in p["b"]] == [1, 4, 9, 7]
    assert _prog_plan(probe, scans, pipeline_max=4)["pipelined"] == 1
    # split: a launch per level and kind -- in level 1 the DC refinement (kind 19000) stands in front of luma 1..5 (kind 100015)
    p = _prog_plan(probe, scans, pipeline=0, split=1)
    assert [x[0] for x in p["b"]] == [1, 9, 4, 7] and p["cut"] == [0, 1, 2, 3, 4]


def test_progressive_plan_refusals(probe):
    scans = _three_files()
    scans[7].level = 64
    assert _prog_plan(probe, scans) == -1
    scans[7].level = -1
    assert _prog_plan(probe, scans) == -1
    scans = _three_files()
    scans[2].cmpc = 5                                                 # a sequential scan of five components
    assert _prog_plan(probe, scans) == -1
    scans[2].cmpc = 0
    assert _prog_plan(probe, scans) == -1
    # twenty scans of 2^31 - 1 intervals in 2^27 - 16 bytes, floor 1: 17 intervals to a piece, 126,322,568 pieces each -- the
    # seventeenth passes 0x7fffffff
    many = []
    for i in range(20):
        s = _scan(A, i, 0, (0, 0), cmpc=3, rsti=1, flags=RST_TABLE, scan_len=(1 << 27) - 16)
        s.t.mcuc = 0x7fffffff
        many.append(s)
    assert _prog_plan(probe, many, floor=1) == -1
    assert _prog_plan(probe, many[:16], floor=1)["pieces"] == 16 * 126322568
