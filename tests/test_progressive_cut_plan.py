"""prog_dec_plan (lep_scan_decode_plan.h) and a scan flagged LEP_HUFFDEC_EARLY_EOF -- the last scan of a file that ends inside it.  Only the
window form (lep_huffprogdec_win.h) knows the cut: a flagged scan it does not take -- a restart interval, a slot that is not 16-byte
aligned, the form switched off -- goes to NO kernel and is listed as declined, whatever else the launch holds.  Descriptors made up here
(tests/emu/prog_cut_plan_probe.cc), no scan byte is read; every expected list is worked out by hand from the rules."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from lepton_amd import abi  # noqa: E402
from test_scan_decode_plan import _scan, A, B  # noqa: E402

EARLY_EOF, RST_TABLE = 1, 2   # LEP_HUFFDEC_EARLY_EOF, LEP_HUFFDEC_RST_TABLE
WIN, RST = 1, 2               # lephuff::kProgDecWin, kProgDecRst (ProgDecScan::pad)


@pytest.fixture(scope="module")
def probe():
    src, so = os.path.join(ROOT, "tests", "emu", "prog_cut_plan_probe.cc"), os.path.join(ROOT, "tests", "emu", "libprog_cut_plan_probe.so")
    tmp = "%s.%d" % (so, os.getpid())
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, src])
    os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.emu_prog_cut_plan.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    return lib


def _plan(probe, scans, win=1, rst=1, pipeline=0):
    arr = (abi.HuffProgDecScan * len(scans))(*scans)
    out = (C.c_int64 * 1024)()
    n = probe.emu_prog_cut_plan(arr, len(scans), win, rst, pipeline, out, 1024)
    assert n >= 0, n
    it = iter(out[:n])
    pairs = lambda: [(next(it), next(it)) for _ in range(next(it))]   # noqa: E731
    p = dict(b=pairs(), plain=pairs(), rst=pairs())
    p["declined"] = [next(it) for _ in range(next(it))]
    p["seq"] = next(it)
    p["pipelined"] = next(it)
    p["deps"] = list(it)
    return p


def _file(frame, base, last_flags=EARLY_EOF, last_rsti=0, last_scan=0):
    """a file of three scans -- DC of all components, luma 1..5 behind it, luma 1..5 refined behind that; the last one is where the file ends"""
    last = _scan(frame, base + 2, 2, (1, 5), sah=1, rsti=last_rsti, flags=last_flags)
    last.t.scan = last_scan
    return [_scan(frame, base, 0, (0, 0), cmpc=3), _scan(frame, base + 1, 1, (1, 5)), last]


def test_a_cut_scan_the_window_form_takes(probe):
    p = _plan(probe, _file(A, 10) + _file(B, 20, last_flags=0))
    # level by level, stable: A's and B's DC scans, their first stages, their refinements -- all on the window form, the flag changes nothing
    assert p["b"] == [(10, WIN), (20, WIN), (11, WIN), (21, WIN), (12, WIN), (22, WIN)]
    assert p["declined"] == [] and p["plain"] == [] and p["rst"] == [] and p["seq"] == 0


def test_a_cut_scan_with_a_restart_interval_goes_to_no_kernel(probe):
    # file A ends inside a scan that has a restart interval (no marker table): prog_win_takes says no, and the older form, which would take
    # an unflagged scan like it (file B's: pad 0), must not see this one
    p = _plan(probe, _file(A, 10, last_rsti=4) + _file(B, 20, last_flags=0, last_rsti=4))
    assert p["declined"] == [12]
    assert p["b"] == [(10, WIN), (20, WIN), (11, WIN), (21, WIN), (22, 0)]
    assert p["plain"] == [] and p["rst"] == []
    # ... nor the interval form, were the scan to carry a marker table: the file is not one of part c's on its account
    p = _plan(probe, _file(A, 10, last_flags=EARLY_EOF | RST_TABLE, last_rsti=4))
    assert p["declined"] == [12] and p["b"] == [(10, WIN), (11, WIN)] and p["plain"] == [] and p["rst"] == []


def test_a_cut_scan_the_window_form_refuses_goes_to_no_kernel(probe):
    # a slot that is not 16-byte aligned
    p = _plan(probe, _file(A, 10, last_scan=0x1001))
    assert p["declined"] == [12] and p["b"] == [(10, WIN), (11, WIN)]
    # the window form switched off (LEP_HUFFPROGDEC_WIN=0): the whole file's other scans go to the older form, the cut one to none
    p = _plan(probe, _file(A, 10) + _file(B, 20, last_flags=0), win=0)
    assert p["declined"] == [12]
    assert p["b"] == [(10, 0), (20, 0), (11, 0), (21, 0), (22, 0)]
    # 2^27 bytes and more
    big = _file(A, 10)
    big[2].t.scan_len = 1 << 27
    assert _plan(probe, big)["declined"] == [12]


def test_nobody_waits_for_a_declined_scan(probe):
    # the one pipelined launch: the scans that are left follow each other as before.  Launch order 10, 20, 11, 21, 22: B's refinement (index
    # 4) follows B's first stage of the same band (index 3); a DC scan and a band 1..5 do not meet, so nothing else follows anything
    p = _plan(probe, _file(A, 10, last_rsti=4) + _file(B, 20, last_flags=0), pipeline=1)
    assert p["declined"] == [12] and p["pipelined"] == 1
    assert p["b"] == [(10, WIN), (20, WIN), (11, WIN), (21, WIN), (22, WIN)]
    assert p["deps"] == [-1] * 16 + [3, -1, -1, -1]
