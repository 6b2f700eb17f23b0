"""lep_enc5_plan.h -- the encoder's knobs as lep_gpu_create reads them from the environment, enc_choice (which encoder a launch takes) and
the split-phase encoder's writer plan, the host code that launch<false>, launch_enc5 and launch_enc5_writer follow -- through
tests/emu/enc5_plan_probe.cc, which sets the variables in its own process for the length of a call.  Every expected number below is worked
out by hand from the rules, none is taken from the functions:
  writer = `after` up to LEP_ENC5_WMAXSEG (4096) segments, LEP_ENC5_WSCHED (after) beyond;
  after:  K = 1, doubled while 2K <= LEP_ENC5_WCHUNKS (64) and segments * 2K <= LEP_ENC5_WLANES (131072); K >= 2: stitched, K records per
          segment, gather in ONE part unless LEP_ENC5_PARTS was given, reported as (1, K); else the lane writer;
  beside: LEP_ENC5_WPARTCHUNKS (4) chunks per part, parts * chunks records per segment, reported as (parts, chunks);
  lane:   clamp(LEP_ENC5_PARTS (8), 1, 8) parts, no records, reported as (0, 0) -- also what a chunked plan degrades to without its records;
  grids:  groups = ceil(segments / 64), lane_groups = ceil(segments * chunks / 64).
One row of the issue's table does not follow from these rules: LEP_ENC5_WLANES=32 at 4 segments was listed as K = 4, but 4 * 2 * 4 = 32 is
not above 32, so the loop doubles once more: K = 8, 32 chunk lanes -- as 2048 segments take K = 64 (131072 lanes) and 65536 take K = 2 in
the same table.  The row stands here with 8, and LEP_ENC5_WLANES=16 is the setting that gives 4."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANE, STITCHED, PART_CHUNKS = 0, 1, 2     # LEP_DEBUG_WRITE_* (include/lepton_mi355x.h)
FIELDS = ("split_phase", "waves", "form", "gather_parts", "chunks", "records", "groups", "lane_groups", "report_parts", "report_chunks", "beside_name")
KNOBS = ("wsched", "wpartchunks", "enc5_waves", "enc_waves", "pair_max", "parts", "parts_given", "scratch_max")
BESIDE = ["LEP_ENC5_WSCHED=beside", "LEP_ENC5_WMAXSEG=0", "LEP_ENC5_PARTS=8", "LEP_ENC5_WPARTCHUNKS=4"]


@pytest.fixture(scope="module")
def probe():
    src, so = os.path.join(ROOT, "tests", "emu", "enc5_plan_probe.cc"), os.path.join(ROOT, "tests", "emu", "libenc5_plan_probe.so")
    tmp = "%s.%d" % (so, os.getpid())
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-o", tmp, src])
    os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.emu_enc5_plan.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]
    lib.emu_enc5_plan.restype = None
    lib.emu_enc5_knobs.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_uint64)]
    lib.emu_enc5_knobs.restype = None
    return lib


def plan(probe, settings, nseg, degraded=False):
    arr, out = (C.c_char_p * max(len(settings), 1))(*[s.encode() for s in settings]), (C.c_int32 * len(FIELDS))()
    probe.emu_enc5_plan(arr, len(settings), nseg, int(degraded), out)
    return dict(zip(FIELDS, out))


def knobs(probe, *settings):
    arr, out = (C.c_char_p * max(len(settings), 1))(*[s.encode() for s in settings]), (C.c_uint64 * len(KNOBS))()
    probe.emu_enc5_knobs(arr, len(settings), out)
    return dict(zip(KNOBS, out))


def writer(p):
    return p["form"], p["gather_parts"], p["chunks"], p["records"], (p["report_parts"], p["report_chunks"])


def stitched(K, gather_parts=1):
    return STITCHED, gather_parts, K, K, (1, K)


def lane(parts=8):
    return LANE, parts, 0, 0, (0, 0)


def test_default_knobs_by_launch_size(probe):
    p = plan(probe, [], 8)
    assert writer(p) == stitched(64) and (p["groups"], p["lane_groups"]) == (1, 8) and not p["beside_name"]     # 8 * 64 / 64 lanes' groups
    p = plan(probe, [], 1024)
    assert writer(p) == stitched(64) and (p["groups"], p["lane_groups"]) == (16, 1024)
    p = plan(probe, [], 2048)                                    # 2048 * 64 = 131072: just inside
    assert writer(p) == stitched(64) and (p["groups"], p["lane_groups"]) == (32, 2048)
    p = plan(probe, [], 2049)                                    # 2049 * 64 = 131136: one step back; ceil(2049 / 64), ceil(65568 / 64)
    assert writer(p) == stitched(32) and (p["groups"], p["lane_groups"]) == (33, 1025)
    assert writer(plan(probe, [], 4096)) == stitched(32)         # 4096 * 32 = 131072
    assert writer(plan(probe, [], 8192)) == stitched(16)         # beyond LEP_ENC5_WMAXSEG the default schedule is `after` all the same
    assert writer(plan(probe, [], 65536)) == stitched(2)         # 65536 * 2 = 131072
    p = plan(probe, [], 65537)                                   # not even two chunks per segment: lane per segment beside gather
    assert writer(p) == lane(8) and (p["groups"], p["lane_groups"]) == (1025, 0) and not p["beside_name"]


def test_chunk_and_lane_limits(probe):
    for nseg in (100, 5000):
        assert writer(plan(probe, ["LEP_ENC5_WCHUNKS=0"], nseg)) == lane(8)
        assert writer(plan(probe, ["LEP_ENC5_WCHUNKS=1"], nseg)) == lane(8)
    p = plan(probe, ["LEP_ENC5_WCHUNKS=4"], 8)
    assert writer(p) == stitched(4) and (p["groups"], p["lane_groups"]) == (1, 1)
    assert writer(plan(probe, ["LEP_ENC5_WCHUNKS=5"], 8)) == stitched(4)         # a power of two
    assert writer(plan(probe, ["LEP_ENC5_WLANES=32"], 4)) == stitched(8)         # 4 * 8 = 32 lanes (the module's docstring)
    assert writer(plan(probe, ["LEP_ENC5_WLANES=31"], 4)) == stitched(4)
    assert writer(plan(probe, ["LEP_ENC5_WLANES=16"], 4)) == stitched(4)
    assert writer(plan(probe, ["LEP_ENC5_WLANES=8"], 4)) == stitched(2)
    assert writer(plan(probe, ["LEP_ENC5_WLANES=7"], 4)) == lane(8)             # 4 * 2 > 7


def test_parts(probe):
    # LEP_ENC5_PARTS holds for a stitched launch's gather; its records are still one part's
    assert writer(plan(probe, ["LEP_ENC5_PARTS=3"], 100)) == stitched(64, 3)
    assert writer(plan(probe, ["LEP_ENC5_PARTS=3"], 5000)) == stitched(16, 3)    # 5000 * 16 = 80000, 5000 * 32 = 160000
    assert writer(plan(probe, ["LEP_ENC5_PARTS=0"], 100)) == stitched(64, 1)
    assert writer(plan(probe, ["LEP_ENC5_PARTS=-4"], 100)) == stitched(64, 1)
    assert writer(plan(probe, ["LEP_ENC5_PARTS=20"], 100)) == stitched(64, 8)
    for nseg in (100, 5000):
        assert writer(plan(probe, ["LEP_ENC5_PARTS=0", "LEP_ENC5_WCHUNKS=0"], nseg)) == lane(1)
        assert writer(plan(probe, ["LEP_ENC5_PARTS=20", "LEP_ENC5_WCHUNKS=0"], nseg)) == lane(8)
        assert writer(plan(probe, ["LEP_ENC5_PARTS=5", "LEP_ENC5_WCHUNKS=0"], nseg)) == lane(5)


def test_schedules(probe):
    assert writer(plan(probe, ["LEP_ENC5_WSCHED=beside"], 100)) == stitched(64)          # LEP_ENC5_WMAXSEG (4096) holds
    assert writer(plan(probe, ["LEP_ENC5_WSCHED=beside"], 4096)) == stitched(32)
    assert writer(plan(probe, ["LEP_ENC5_WSCHED=beside"], 4097)) == (PART_CHUNKS, 8, 4, 32, (8, 4))
    assert writer(plan(probe, ["LEP_ENC5_WSCHED=lane"], 4097)) == lane(8)
    for nseg, grids in ((100, (2, 7)), (5000, (79, 313))):         # ceil(100 / 64), ceil(400 / 64); ceil(5000 / 64), ceil(20000 / 64)
        p = plan(probe, BESIDE, nseg)
        assert writer(p) == (PART_CHUNKS, 8, 4, 32, (8, 4)) and (p["groups"], p["lane_groups"]) == grids and p["beside_name"]
        assert writer(plan(probe, ["LEP_ENC5_WSCHED=lane", "LEP_ENC5_WMAXSEG=0"], nseg)) == lane(8)
        assert writer(plan(probe, ["LEP_ENC5_WSCHED=after", "LEP_ENC5_WMAXSEG=0"], nseg)) == stitched(64 if nseg == 100 else 16)
    p = plan(probe, ["LEP_ENC5_WSCHED=2", "LEP_ENC5_WMAXSEG=0", "LEP_ENC5_PARTS=2", "LEP_ENC5_WPARTCHUNKS=8"], 100)
    assert writer(p) == (PART_CHUNKS, 2, 8, 16, (2, 8)) and p["lane_groups"] == 13 and p["beside_name"]       # ceil(800 / 64)
    assert writer(plan(probe, ["LEP_ENC5_WSCHED=beside", "LEP_ENC5_WMAXSEG=0", "LEP_ENC5_WCHUNKS=0"], 100)) == (PART_CHUNKS, 8, 4, 32, (8, 4))   # (the stitched writer's knob)


def test_plan_without_room_for_the_records(probe):
    """the lane writer in LEP_ENC5_PARTS parts -- not in the one part the stitched plan had"""
    for nseg in (8, 100, 5000):
        assert writer(plan(probe, [], nseg))[:2] == (STITCHED, 1) and writer(plan(probe, [], nseg, degraded=True)) == lane(8)
        assert writer(plan(probe, ["LEP_ENC5_PARTS=3"], nseg, degraded=True)) == lane(3)
        assert writer(plan(probe, BESIDE, nseg, degraded=True)) == lane(8)
        assert not plan(probe, BESIDE, nseg, degraded=True)["beside_name"]
    assert writer(plan(probe, ["LEP_ENC5_WSCHED=beside", "LEP_ENC5_WMAXSEG=0", "LEP_ENC5_PARTS=2"], 100, degraded=True)) == lane(2)


def test_encoder_choice(probe):
    choice = lambda settings, nseg: (bool(plan(probe, settings, nseg)["split_phase"]), plan(probe, settings, nseg)["waves"])
    assert choice([], 7) == (False, 2) and choice([], 8) == (True, 2)
    assert choice(["LEP_ENC5_MIN=0"], 8) == (False, 2) and choice(["LEP_ENC5_MIN=0"], 100000) == (False, 8)
    assert choice(["LEP_ENC5_MIN=1"], 1) == (True, 2) and choice(["LEP_ENC5_MIN=64"], 63) == (False, 2) and choice(["LEP_ENC5_MIN=64"], 64) == (True, 2)
    assert choice(["LEP_ENC_WAVES=4"], 8) == (False, 4) and choice(["LEP_ENC_WAVES=4"], 100000) == (False, 4)
    assert choice(["LEP_ENC_WAVES=2"], 100000) == (False, 2) and choice(["LEP_ENC_WAVES=8"], 8) == (False, 8)
    assert choice(["LEP_ENC_WAVES=3"], 8) == (True, 2)             # not a form: as if unset
    # the form behind the split-phase encoder: v3x2 up to LEP_ENC_PAIR_MAX (1280), v3<4> up to 4608, v3<8> above
    assert [choice([], n) for n in (1280, 1281, 4608, 4609)] == [(True, 2), (True, 4), (True, 4), (True, 8)]
    assert [choice(["LEP_ENC_PAIR_MAX=100"], n)[1] for n in (100, 101)] == [2, 4]
    assert choice(["LEP_ENC_PAIR_MAX=10000"], 4609) == (True, 8)


def test_knobs_from_the_environment(probe):
    d = knobs(probe)
    assert d == dict(wsched=1, wpartchunks=4, enc5_waves=2, enc_waves=0, pair_max=1280, parts=8, parts_given=0, scratch_max=2 ** 64 - 1)
    assert [knobs(probe, "LEP_ENC5_WSCHED=" + v)["wsched"] for v in ("lane", "after", "beside", "0", "1", "2", "7", "-3", "else")] == [0, 1, 2, 0, 1, 2, 2, 0, 0]
    assert [knobs(probe, "LEP_ENC5_WPARTCHUNKS=%d" % v)["wpartchunks"] for v in (0, 1, 2, 3, 4, 31, 32, 33, 100, -5)] == [1, 1, 2, 2, 4, 16, 32, 32, 32, 1]
    assert [knobs(probe, "LEP_ENC5_WAVES=%d" % v)["enc5_waves"] for v in (0, 1, 2, 3)] == [2, 1, 2, 2]
    assert [knobs(probe, "LEP_ENC_WAVES=%d" % v)["enc_waves"] for v in (0, 2, 3, 4, 8, 16)] == [0, 2, 0, 4, 8, 0]
    d = knobs(probe, "LEP_ENC5_PARTS=3", "LEP_ENC5_SCRATCH_MAX=123456789012")
    assert (d["parts"], d["parts_given"], d["scratch_max"]) == (3, 1, 123456789012)
    assert knobs(probe, "LEP_ENC5_PARTS=8")["parts_given"] == 1      # given, even where it names the default


def test_the_probe_leaves_the_environment_alone(probe, monkeypatch):
    monkeypatch.setenv("LEP_ENC5_WCHUNKS", "4")      # (os.environ: putenv, i.e. the C environment the probe reads)
    assert writer(plan(probe, [], 8)) == stitched(64)               # only the call's own settings count ...
    getenv = C.CDLL(None).getenv
    getenv.argtypes, getenv.restype = [C.c_char_p], C.c_char_p
    assert getenv(b"LEP_ENC5_WCHUNKS") == b"4"                      # ... and what was there is there again
