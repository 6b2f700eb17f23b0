"""The gather pass of the split-phase encoder stages a lane's bins in a ring of 64 and lets the lanes write their complete sectors together
at check points (lep_enc5.h Walk5::put_bin / drain / flush_bin).  Stepped on the CPU through tests/emu/enc5_gather_emu.cc -- count -> plan ->
emit -> bucket -> fold -> gather -> write, with one wavefront, with the walks' two halves and with gather in seven parts -- on frames made
to stress the staging (tests/enc5_gather_frames.py): every segment's stream and bin count are the oracle's, the ring's invariant holds
(exit code 1008 otherwise), nothing is written behind the bins, and the bin list equals the one of the form before
(-DLEP_ENC5_GATHER_ROW_FLUSH=0) half word for half word."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
from conftest import ROOT
from enc5_gather_frames import CONTENTS, SHAPES, frame
from lepton_amd import abi

POISON = 0xA5A5
FORMS = ((1, 1), (2, 1), (1, 7))   # (wavefronts per segment, parts): one wavefront; the two halves; gather in seven parts


def _build(name, flags):
    src = os.path.join(ROOT, "tests", "emu", "enc5_gather_emu.cc")
    so = os.path.join(ROOT, "tests", "emu", "libcore_emu_enc5gather%s.so" % name)
    tmp = "%s.%d" % (so, os.getpid())
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared"] + flags + ["-o", tmp, src])
    os.replace(tmp, so)
    L = C.CDLL(so)
    L.emu_enc5_gather.argtypes = [C.POINTER(abi.ImageDesc), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32),
                                  C.POINTER(C.c_uint32), C.POINTER(C.c_uint16), C.c_uint32, C.POINTER(C.c_uint32)]
    return L


@pytest.fixture(scope="module")
def emus():
    new, old = _build("_row_flush", []), _build("_before", ["-DLEP_ENC5_GATHER_ROW_FLUSH=0"])
    assert new.emu_enc5_gather_knobs() == 1, "the emulation was not built with the staging ring"
    assert old.emu_enc5_gather_knobs() == 0
    return new, old


def run(L, d, s, waves, parts, cap):
    """(exit code, stream, bins, the bin list with the room behind it)"""
    out = C.create_string_buffer(cap)
    n, nb, ll = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    lcap = 1 << 22
    lst = np.zeros(lcap, np.uint16)
    rc = L.emu_enc5_gather(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, waves, parts, out, cap, C.byref(n), C.byref(nb),
                           lst.ctypes.data_as(C.POINTER(C.c_uint16)), lcap, C.byref(ll))
    assert ll.value <= lcap
    return rc, out.raw[:n.value], nb.value, lst[:ll.value]


def check(emus, img, segs):
    new, old = emus
    d = img.desc
    want, bins = ob.oracle_encode(d, segs)
    total = 0
    for s, w in zip(segs, want):
        first = None
        for waves, parts in FORMS:
            rc, got, nb, lst = run(new, d, s, waves, parts, len(w) + 4096)
            assert rc == 0, (waves, parts, rc)   # (1008: a bin put on a staged slot that had not been written)
            assert got == w, (waves, parts)
            assert (lst[nb:] == POISON).all(), (waves, parts, int(np.flatnonzero(lst[nb:] != POISON)[0]))
            rc0, got0, nb0, lst0 = run(old, d, s, waves, parts, len(w) + 4096)
            assert rc0 == 0 and got0 == w and nb0 == nb
            assert np.array_equal(lst, lst0), (waves, parts, int(np.flatnonzero(lst != lst0)[0]))
            if first is None:
                first = (nb, lst)
            assert nb == first[0] and np.array_equal(lst, first[1])
        total += first[0]
    assert total == bins


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_%s" % (s[0], s[1], "one_component" if s[2] else "420"))
def test_gather_bins_equal_the_oracle_and_the_form_before(emus, shape, content):
    img = frame(*shape, content)
    check(emus, img, img.plan())


@pytest.mark.parametrize("content", ["alternating", "empty_beside_dense"])
def test_segment_that_starts_below_the_first_row(emus, content):
    """two segments of a 65 x 4 frame: the second starts at luma row 2 -- its first tile has no row above in the segment, its bins start at 0"""
    img = frame(65, 4, False, content)
    segs = [abi.Segment(0, 0, 2, 0), abi.Segment(0, 2, 4, 1)]
    check(emus, img, segs)


def test_dense_frame_reaches_the_bound(emus):
    """the dense frame is the bound the ring is sized for: its coefficients take 22 bins each, so lanes do hold two complete sectors
    (more than 64 bins between two writes would be exit code 1008, checked above; here: the frame really is that dense)"""
    img = frame(64, 2, True, "dense")
    d = img.desc
    _, bins = ob.oracle_encode(d, img.plan())
    assert bins >= d.nblocks(0) * (63 * 22 + 12)
