"""simt_stuff_bytes (lep_huff_simt.h) -- the stuffing loop the two lane-per-unit scan writers share -- on made-up bit buffers, as a
lane-loop emulation (tests/emu/prog_simt_rst_emu.cc emu_simt_stuff_bytes) against a byte loop: a 00 behind every FF the marker map does
not name, 16 bytes per lane, 1024 per step, clipped to cap."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [15, 16, 17, 1023, 1024, 1025, 2049]


@pytest.fixture(scope="module")
def emu():
    src, so = os.path.join(ROOT, "tests", "emu", "prog_simt_rst_emu.cc"), os.path.join(ROOT, "tests", "emu", "libprog_simt_rst_emu_backend.so")
    tmp = "%s.%d" % (so, os.getpid())
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, src])
    os.replace(tmp, so)
    lib = C.CDLL(so)
    lib.emu_simt_stuff_bytes.restype = C.c_uint32
    lib.emu_simt_stuff_bytes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
    return lib


def _want(data, marked):
    out = bytearray()
    for i, b in enumerate(data):
        out.append(b)
        if b == 0xFF and i not in marked:
            out.append(0)
    return bytes(out)


def _run(emu, data, marked, cap, with_map=True):
    """(written, the bytes below cap, whether everything from cap on is untouched)"""
    nb = len(data)
    padded = bytes(data) + b"\x5a" * (-nb % 16 + 16)                 # the loop reads a lane's 16 bytes whole
    buf = np.frombuffer(padded, dtype=">u4").astype(np.uint32)      # byte i of the stream: bits 31-8(i & 3) .. of dword i >> 2
    bits = np.zeros(len(padded) // 32 + 2, dtype=np.uint32)         # bit q of the map: byte q is a restart marker's FF
    for q in marked:
        bits[q >> 5] |= np.uint32(1 << (q & 31))
    room = max(cap, 2 * nb) + 8
    out = np.full(room, 0xA5, dtype=np.uint8)
    written = emu.emu_simt_stuff_bytes(buf.ctypes.data, nb, bits.ctypes.data if with_map else None, out.ctypes.data, cap)
    return written, out[:min(cap, room)].tobytes(), bool((out[cap:] == 0xA5).all())


def _check(emu, data, marked, caps, with_map=True):
    want = _want(data, marked if with_map else ())
    for cap in caps:
        written, got, untouched = _run(emu, data, marked, cap, with_map)
        assert written == len(want), (len(data), cap, written, len(want))
        assert got[:min(cap, len(want))] == want[:cap], (len(data), cap)
        assert got[len(want):] == b"\xa5" * max(0, cap - len(want)) and untouched, (len(data), cap, "written at or past cap, or past the stream's end")


@pytest.mark.parametrize("nb", SIZES)
def test_stuffing_against_a_byte_loop(emu, nb):
    """every size around a lane's 16 bytes and a step's 1024: an FF as the last byte of a lane's 16 and as the first of the next, at bytes
    1023 and 1024, as the stream's last byte; marker bits in the low and in the high half of a map word, on an FF beside an unmarked FF;
    cap = 0, cap between an FF and its 00, cap at and past the end; no marker map at all"""
    rng = np.random.default_rng(nb)
    data = bytearray(int(x) for x in rng.integers(0, 255, nb))      # (no FF but the ones put there)
    ffs = [p for p in (3, 4, 15, 16, 17, 31, 32, 47, 48, 49, 1007, 1008, 1022, 1023, 1024, 1025, 1039, 1040, 2047, 2048, nb - 1) if 0 <= p < nb]
    for p in ffs:
        data[p] = 0xFF
    # marked: 4, 15, 1024, 2048 (bits 4, 15, 0, 0 of their map words: the low half, i & 16 = 0) and 48, 1008 (bit 16: the high half) -- the FFs
    # at 3, 16, 47, 49, 1007, 1023, 1025, 2047 beside them stay unmarked
    marked = {p for p in (4, 15, 48, 1008, 1024, 2048) if p < nb}
    want = _want(data, marked)
    first_ff = next(i for i, b in enumerate(want) if b == 0xFF and i + 1 < len(want) and want[i + 1] == 0)
    caps = sorted({0, 1, first_ff, first_ff + 1, first_ff + 2, len(want) - 1, len(want), len(want) + 5} | {c for c in (16, 17, 1024, 1025, 1030) if c < len(want)})
    _check(emu, bytes(data), marked, caps)
    _check(emu, bytes(data), marked, [0, first_ff + 1, len(want) + 40], with_map=False)     # marker_map = nullptr: every FF takes its 00
    _check(emu, b"\xff" * nb, set(), [0, 1, nb, 2 * nb - 1, 2 * nb])                           # nothing but FFs: the prefix sum carries 16 per lane
    _check(emu, b"\xff" * nb, set(range(nb)), [nb - 1, nb])                                 # ... all of them markers: none takes a 00
