"""Interleaved scans in which every block uses the same DC and the same AC table and the MCU has MORE than four blocks -- 4:2:0 written
with one pair of tables is six -- on the lane-per-subsequence scan decoder (lep_huffdec_simt.h simt_blind_phases), stepped on the CPU.

Which block of the MCU a lane stands on is not in the bits of such a scan.  With 2 .. 4 blocks per MCU the lanes have summed their DC
differences per SLOT since round 6 (SimtSub::dcsum); wider MCUs answered status 3 after three wasted settle passes and took the
single-wave kernel.  Their slot sums now go through a column of LDS per lane into a side array (SimtSlots) and pass P rotates them into
component sums exactly as it does the four of SimtSub.  Everything here is held against the single-wave emulation
(emu_huffman_decode_image): "agree" = the frame, every row record and the final record are identical.

The passes are stepped by tests/emu/blind_wide_emu.cc (core_emu.cc plus emu_huffman_decode_image_simt_slots), which hands them the side
array and the columns as the launch code hands them to the kernels; core_emu.cc's own driver passes none, and to a caller without
the array such an image is what it always was (the last test).

On the commit before this one every case of five and more blocks per MCU ends with status 3 (run there through core_emu.cc's driver,
the six-block ones included: all red); the three- and four-block layouts are the regression anchors."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# (component id, h, v, quantisation table, DC table, AC table): tables 0 / 0 for every component
LAYOUTS = {
    "3_444": [(1, 1, 1, 0, 0, 0), (2, 1, 1, 0, 0, 0), (3, 1, 1, 0, 0, 0)],                 # anchors: SimtSub::dcsum holds their sums
    "4_y21_c_c": [(1, 2, 1, 0, 0, 0), (2, 1, 1, 0, 0, 0), (3, 1, 1, 0, 0, 0)],
    "5_y22_c": [(1, 2, 2, 0, 0, 0), (2, 1, 1, 0, 0, 0)],
    "6_420": [(1, 2, 2, 0, 0, 0), (2, 1, 1, 0, 0, 0), (3, 1, 1, 0, 0, 0)],
    "6_y21_cb21_cr21": [(1, 2, 1, 0, 0, 0), (2, 2, 1, 0, 0, 0), (3, 2, 1, 0, 0, 0)],
    "8_y22_cb21_cr21": [(1, 2, 2, 0, 0, 0), (2, 2, 1, 0, 0, 0), (3, 2, 1, 0, 0, 0)],
    "10_y22_cb22_cr21": [(1, 2, 2, 0, 0, 0), (2, 2, 2, 0, 0, 0), (3, 2, 1, 0, 0, 0)],
    "12_y22_cb22_cr22": [(1, 2, 2, 0, 0, 0), (2, 2, 2, 0, 0, 0), (3, 2, 2, 0, 0, 0)],      # the most the parser passes: three components, 2 x 2 each
}
MUST_BE_ELIGIBLE = ("3_444", "4_y21_c_c", "5_y22_c", "6_420", "6_y21_cb21_cr21")
# (width, height, bits per subsequence): the first has more than 64 subsequences -- the prefix sums cross 64-lane groups -- and the last
# is the product's order of magnitude.
#
# The files.  The assertion on the second settle pass needs every lane to fall into step with the block boundaries inside ONE
# subsequence.  That is a matter of the bits alone and has nothing to do with slots: a lane that guesses from mid-code decodes nonsense
# until a code boundary happens to fit, and one nonsense block can run over several hundred bits.  At 1024 bits no lane of 72 files drawn
# for this test overshot; at 512 bits about one lane in 500 does whatever the layout -- the three-block anchor, which the commit before
# this one decodes the same way, moves in its second settle pass for 3 files in 12 at density 0.02 and for 8 in 12 at 0.1 (333 x 250) --
# and the lane behind it then needs the second pass.  So the 512-bit files are drawn with short blocks (density 0.02: some 18 bits, 28 to
# a subsequence) and with fixed seeds, the first of the series 1000 k + 7 w + h for which the layout's file settles in one pass (k = 1 for
# two layouts at 333 x 250, k = 0 for everything else).  This cannot hide what the assertion is there to catch: a slot that travels lane
# by lane moves in EVERY settle pass of EVERY file with more than a few subsequences, whatever its seed.
SIZES = [(640, 480, 1024), (333, 250, 512), (97, 50, 512), (640, 480, 32768)]
DENSITY = 0.02          # the wrap, cut and restart files, and the 512-bit subsequences below


def _file_for(layout, w, h, sub_bits):
    import jpeg_writer as jw

    comps = LAYOUTS[layout]
    k = 1 if (w, h, sub_bits) == (333, 250, 512) and layout in ("6_y21_cb21_cr21", "8_y22_cb21_cr21") else 0
    return jw.write_baseline(w, h, comps, np.random.default_rng(1000 * k + 7 * w + h), density=DENSITY if sub_bits == 512 else 0.1)[0]


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "blind_wide_emu.cc")
    so = os.path.join(ROOT, "tests", "emu", "libcore_emu_blindwide.so")
    tmp = "%s.%d" % (so, os.getpid())
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, src])
    os.replace(tmp, so)
    return C.CDLL(so)


class _WithSlots:
    """the emulation library with emu_huffman_decode_image_simt standing for the driver that passes the side array (for helpers of
    test_core_emulation, which call it by that name)"""

    def __init__(self, lib):
        self._lib = lib
        self.emu_huffman_decode_image_simt = lib.emu_huffman_decode_image_simt_slots

    def __getattr__(self, name):
        return getattr(self._lib, name)


def _open(jpg, with_restart_table=False):
    """lep_jpeg_open_gpu + a zero padded copy of the scan (the marker table behind it on request) + zeroed planes; None = not eligible"""
    from lepton_amd import abi

    L = abi.lib()
    h = C.c_void_p()
    img = abi.HuffDecImage()
    ok = C.c_int(0)
    assert L.lep_jpeg_open_gpu(jpg, len(jpg), C.byref(h), C.byref(img), C.byref(ok)) == 0
    if not ok.value:
        L.lep_jpeg_close(h)
        return None
    p, n = C.c_void_p(), C.c_size_t(0)
    L.lep_jpeg_scan_bytes(h, C.byref(p), C.byref(n))
    table = b""
    if with_restart_table:
        rp, rn = C.POINTER(C.c_uint32)(), C.c_size_t(0)
        L.lep_jpeg_scan_restarts(h, C.byref(rp), C.byref(rn))
        assert rn.value == (img.mcuc - 1) // img.rsti and rn.value > 0
        table = bytes(C.cast(rp, C.POINTER(C.c_uint8 * (4 * rn.value))).contents)
    room = (n.value + 64 + 15) & ~15
    scan = C.create_string_buffer(C.string_at(p, n.value) + bytes(room - n.value) + table + bytes(64), room + len(table) + 64)
    assert C.addressof(scan) % 8 == 0
    img.scan = C.addressof(scan)
    planes = [C.create_string_buffer(img.bch[c] * img.vs[c] * img.mcuv * 128) for c in range(img.ncomp)]
    for c in range(img.ncomp):
        img.blocks[c] = C.cast(planes[c], C.c_void_p).value
    return img, scan, planes, h


def _records(rows):
    return [(r.bitpos, tuple(r.last_dc), r.aux) for r in rows]


def _both(emu, jpg, sub_bits, with_restart_table=False, old_driver=False):
    """the single-wave emulation, then the lane-per-subsequence one into the same (wiped) planes:
    (single-wave frame, its records, lane frame, lane records, settle_moved, nsub, image)"""
    from lepton_amd import abi

    one = _open(jpg, with_restart_table)
    assert one is not None
    img, scan, planes, h = one
    abi.lib().lep_jpeg_close(h)
    rows1 = (abi.HuffDecRow * (img.mcuv + 1))()
    assert emu.emu_huffman_decode_image(C.byref(img), rows1) == 0
    want = [p.raw for p in planes]
    for p in planes:
        C.memset(p, 0, len(p))
    rows2 = (abi.HuffDecRow * (img.mcuv + 1))()
    moved, nsub = (C.c_int32 * 8)(), C.c_uint32(0)
    decode = emu.emu_huffman_decode_image_simt if old_driver else emu.emu_huffman_decode_image_simt_slots
    assert decode(C.byref(img), rows2, sub_bits, moved, C.byref(nsub)) == 0
    return want, _records(rows1), [p.raw for p in planes], _records(rows2), list(moved)[:4], nsub.value, img


def _agrees(emu, jpg, sub_bits, what, with_restart_table=False):
    want, rec1, got, rec2, moved, nsub, img = _both(emu, jpg, sub_bits, with_restart_table)
    assert rec1[-1][2] >> 8 == 0, (what, "the single-wave emulation reports an irregular scan")
    status = (rec2[-1][2] >> 8) & 0x3fffff
    assert status == 0, (what, "status", status, "settle passes that moved", moved, "subsequences", nsub)
    assert got == want, (what, "frames differ")
    assert rec2 == rec1, (what, "records differ")
    return moved, nsub


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_blind_images_of_every_slot_count_agree_with_the_single_wave_decoder(emu, layout):
    """status 0, frame and records of the single-wave emulation, and nothing travels lane by lane: with more than four subsequences the
    second settle pass moves no end state"""
    import jpeg_writer as jw

    comps = LAYOUTS[layout]
    crossed = False
    for w, h, sub_bits in SIZES:
        jpg = _file_for(layout, w, h, sub_bits)
        if _open(jpg) is None:
            assert layout not in MUST_BE_ELIGIBLE, (layout, "must be eligible for the GPU scan decoder")
            pytest.skip("not eligible for the GPU scan decoder")
        moved, nsub = _agrees(emu, jpg, sub_bits, (layout, w, h, sub_bits))
        if nsub > 4:
            assert moved[2] == 0, (layout, w, h, sub_bits, "still moving in the second settle pass", moved)
        crossed = crossed or nsub > 64
    assert crossed, "no file had more than 64 subsequences: the prefix sums never crossed a 64-lane group"


def _walking_dc(rng, comps, w, h, amp):
    """blocks whose luma DC alternates between +1000 and -1000 from block to block in scan order: the DC differences of an MCU slot all
    have one sign and 2000 each, so a lane's per-slot sum leaves int16 after seventeen MCUs"""
    import jpeg_writer as jw

    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mcux, mcuy = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    blocks = [jw.random_blocks(rng, mcux * c[1] * mcuy * c[2], DENSITY, amp).reshape(mcuy * c[2], mcux * c[1], 64) for c in comps]
    ph, pv = comps[0][1], comps[0][2]
    k = 0
    for my in range(mcuy):
        for mx in range(mcux):
            for by in range(pv):
                for bx in range(ph):
                    blocks[0][my * pv + by][mx * ph + bx][0] = 1000 if k % 2 == 0 else -1000
                    k += 1
    return blocks


@pytest.mark.parametrize("layout", ["6_420", "10_y22_cb22_cr21"])
def test_slot_sums_that_wrap_int16(emu, layout):
    """large amplitudes, and luma DC differences of +-2000 whose sign goes with the slot: over the few hundred MCUs of a 32768-bit
    subsequence every luma slot sum wraps int16 several times -- the predictors pass P hands to pass C must still be the decoder's"""
    import jpeg_writer as jw

    comps = LAYOUTS[layout]
    rng = np.random.default_rng(420)
    w, h = 640, 480
    blocks = _walking_dc(rng, comps, w, h, amp=600.0)
    jpg, _ = jw.write_baseline(w, h, comps, rng, density=DENSITY, amp=600.0, blocks=blocks)
    if _open(jpg) is None:
        assert layout not in MUST_BE_ELIGIBLE
        pytest.skip("not eligible for the GPU scan decoder")
    for sub_bits in (32768, 8192):
        moved, nsub = _agrees(emu, jpg, sub_bits, (layout, "wrapping sums", sub_bits))
        assert nsub > 4 and moved[2] == 0, (layout, sub_bits, moved, nsub)
        # (the sums do wrap: a subsequence holds more than 17 MCUs of 2000 per luma slot)
        mcus_per_sub = (w // 16) * (h // 16) / nsub
        assert mcus_per_sub * 2000 > 32768, mcus_per_sub


def test_six_block_file_cut_inside_its_scan(emu):
    """A 4:2:0 one-pair file without EOI, cut at bytes inside its scan: the lanes stop at the block that reads the data's last bit and leave
    the truncation record {blocks decoded, DC predictors, LEP_HUFFDEC_ROW_TRUNCATED}, as blind images of 2 .. 4 blocks do.

    What it is held against: the single-wave kernel has no notion of the cut -- it runs out of data inside a block and answers status 2,
    which is why cut files go to the lane kernels and never to it (lep_huffdec.h run; test_core_emulation's cut-file tests) -- so its
    final record is no truncation record to compare with.  The record, the frame and the .lep written from them are therefore held
    against the HOST PARSER's, the reference's reading of a cut file (test_core_emulation's helper, the same that checks the 2 .. 4-slot
    images), and against the single-wave emulation where the two overlap: its status is 2, and every row record in front of the cut
    and every block the lanes decoded but the last (which reads zeros behind the data's end) are its own."""
    import jpeg_writer as jw
    import test_core_emulation as tce
    from lepton_amd import abi

    comps = LAYOUTS["6_420"]
    whole, _ = jw.write_baseline(333, 250, comps, np.random.default_rng(77), density=DENSITY)
    sos = whole.find(b"\xff\xda")
    taken = 0
    for cut in (sos + 14 + (len(whole) - sos) // 3, sos + 14 + (len(whole) - sos) * 3 // 4, len(whole) - 40):
        jpg = whole[:cut]
        for sub_bits in (512, 8192):
            res = tce._cut_file_through_the_lane_per_subsequence_decoder(_WithSlots(emu), jpg, sub_bits)
            assert res is True, (cut, sub_bits, res)                  # status 0, the host parser's frame, hand-offs, bounds and .lep
            taken += 1
        want, rec1, got, rec2, moved, nsub, img = _both(emu, jpg, 512)
        assert img.flags & 1 and (rec1[-1][2] >> 8) & 0x3fffff == 2   # the single-wave emulation: out of data inside a block
        assert (rec2[-1][2] >> 8) & 0x3fffff == 0 and rec2[-1][2] & 0x40000000, (cut, rec2[-1])
        done = rec2[-1][0]                                            # blocks decoded
        assert 0 < done < img.mcuc * 6
        rows_entered = (done - 1) // 6 // img.mcuh + 1
        assert rec2[:rows_entered] == rec1[:rows_entered], cut
        # blocks in front of the last decoded one, in scan order: equal in both frames
        slot = [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (2, 0, 0)]
        for k in (0, done // 2, done - 2):
            mcu, ph = divmod(k, 6)
            c, v, hh = slot[ph]
            row, mx = divmod(mcu, img.mcuh)
            at = ((row * img.vs[c] + v) * img.bch[c] + mx * img.hs[c] + hh) * 128
            assert got[c][at:at + 128] == want[c][at:at + 128], (cut, k)
        assert nsub > 4 and moved[2] == 0, (cut, moved, nsub)
    assert taken == 6


def test_six_block_file_with_restart_intervals_keeps_the_interval_path(emu):
    """restart interval + marker table (LEP_HUFFDEC_RST_TABLE): lane = interval, nothing is guessed and no slot is summed -- the image
    is not blind to the kernels (simt_blind_phases) and its result is the single-wave emulation's, as before"""
    import jpeg_writer as jw

    comps = LAYOUTS["6_420"]
    for w, h, ri in [(333, 250, 5), (640, 480, 1), (97, 50, 3)]:
        jpg, _ = jw.write_baseline(w, h, comps, np.random.default_rng(w + ri), density=DENSITY, restart_interval=ri)
        one = _open(jpg, with_restart_table=True)
        assert one is not None
        assert one[0].flags & 2 and one[0].rsti == ri
        from lepton_amd import abi
        abi.lib().lep_jpeg_close(one[3])
        moved, nsub = _agrees(emu, jpg, 512, (w, h, ri), with_restart_table=True)
        assert nsub == (one[0].mcuc - 1) // ri + 1                    # lanes are intervals, not subsequences of 512 bits


def test_a_caller_without_the_side_array_gets_the_old_answer(emu):
    """core_emu.cc's emu_huffman_decode_image_simt passes no side array: a six-block image is then not taken for blind, and either the
    run agrees with the single-wave emulation or it ends with a status -- never a different result, never a read of an array that is
    not there"""
    answered = 0
    for w, h, sub_bits in SIZES:
        jpg = _file_for("6_420", w, h, sub_bits)
        want, rec1, got, rec2, moved, nsub, img = _both(emu, jpg, sub_bits, old_driver=True)
        if (rec2[-1][2] >> 8) & 0x3fffff:
            answered += 1
            continue
        assert got == want and rec2 == rec1, (w, h, sub_bits)
    assert answered >= 1                                              # (many lanes, no slot knowledge: status 3)
