"""lep_huffprog_simt.h on progressive scans with a restart interval -- written with one lane per run of blocks -- as a lane-loop emulation
(tests/emu/prog_simt_rst_emu.cc: every pass one emulated wavefront after the other, over garbage-filled scratch) against the wavefront
form (lep_huffprog.h through core_emu.cc's emu_huffman_progressive_encode) and against the original files.  No file is skipped: a file the
planner does not take fails its test."""
import ctypes as C
import io
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_binding as ob  # noqa: E402
from conftest import golden, ref_golden  # noqa: E402
from lepton_amd.codec import JpegImage  # noqa: E402

WAVE, LANE, LANE_RST = 0, 1, 2


def _build(src, so):
    tmp = "%s.%d" % (so, os.getpid())
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, src])
    os.replace(tmp, so)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def lanes():
    return _build(os.path.join(ROOT, "tests", "emu", "prog_simt_rst_emu.cc"), os.path.join(ROOT, "tests", "emu", "libprog_simt_rst_emu.so"))


@pytest.fixture(scope="module")
def core():
    """core_emu.cc as it is: emu_huffman_progressive_encode (lep_huffprog.h) is what the new form is held against"""
    return _build(os.path.join(ROOT, "tests", "emu", "core_emu.cc"), os.path.join(ROOT, "tests", "emu", "libcore_emu_progsimtrst.so"))


def _plan(jpg, lep=None, what=None):
    """(file, image, scans, n): the descriptors lep_file_recode_plan_progressive fills, the file's own frame in place.  A file the planner
    does not take is a failure, never a skip."""
    from lepton_amd import abi
    from lepton_amd.codec import LepFile

    src = JpegImage(jpg)
    if lep is None:
        streams, _ = ob.oracle_encode(src.desc, src.plan())
        lep = src.write_lep(streams)
    f = LepFile(lep)
    for c in range(f.desc.ncomp):
        C.memmove(f.desc.blocks[c], src.desc.blocks[c], f.desc.nblocks(c) * 128)
    img = abi.HuffProgImage()
    scans = (abi.HuffProgScan * 64)()
    nscan, ok = C.c_int(0), C.c_int(0)
    assert abi.lib().lep_file_recode_plan_progressive(f.handle, C.byref(img), scans, 64, C.byref(nscan), C.byref(ok)) == 0
    assert ok.value, (what, "the planner does not take this file")
    return f, img, scans, nscan.value


def _interval(img, sc):
    return sc.rsti if sc.rsti >= 0 else img.rsti


def _both_forms(core, lanes, img, scans, n, region=0, rst_on=1):
    """every scan through the wavefront form and through the launch code's routing over the lane forms:
    ([(len, bytes, len, bytes)], taken, the buffers of the lane run)"""
    out_total = corr_total = 0
    for i in range(n):
        scans[i].image = 0
        scans[i].out_off = out_total
        out_total += (scans[i].out_cap + 15) & ~15
        scans[i].corr_off = corr_total
        corr_total += scans[i].corr_cap
    corr = (C.c_uint32 * (corr_total + 8))()
    out0, out1 = C.create_string_buffer(out_total + 64), C.create_string_buffer(out_total + 64)
    len0, len1 = (C.c_uint32 * n)(), (C.c_uint32 * n)()
    core.emu_huffman_progressive_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert core.emu_huffman_progressive_encode(C.byref(img), scans, n, out0, corr, len0) == 0
    taken, intact = (C.c_int32 * n)(), C.c_int32(0)
    lanes.emu_huffman_progressive_encode_lanes.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
    assert lanes.emu_huffman_progressive_encode_lanes(C.byref(img), scans, n, out1, corr, len1, taken, region, rst_on, C.byref(intact)) == 0
    assert intact.value == 1, "a pass wrote outside the region or the unit arrays"
    res = [(len0[i], out0.raw[scans[i].out_off: scans[i].out_off + (len0[i] & 0x7fffffff)],
            len1[i], out1.raw[scans[i].out_off: scans[i].out_off + (len1[i] & 0x7fffffff)]) for i in range(n)]
    return res, list(taken), (out1, len1)


def _three_assertions(core, lanes, jpg, lep=None, what=None, want_intervals=True):
    """every scan with an interval is taken by the new form; every scan's bytes and length are the wavefront form's; the glued file is the
    original.  Returns how many scans the new form took and how many restart markers they hold."""
    from lepton_amd import abi

    L = abi.lib()
    f, img, scans, n = _plan(jpg, lep, what)
    res, taken, (out1, len1) = _both_forms(core, lanes, img, scans, n)
    for i in range(n):
        assert taken[i] == (LANE_RST if _interval(img, scans[i]) != 0 else LANE), (what, i, taken, _interval(img, scans[i]))
    for i, (l0, b0, l1, b1) in enumerate(res):
        assert l0 < 0x80000000, (what, i, "the wavefront form outgrew its slot")
        assert l1 == l0 and b1 == b0, (what, i, scans[i].from_, scans[i].to, scans[i].sah, scans[i].sal, _interval(img, scans[i]), l0, l1,
                                       next((k for k in range(min(len(b0), len(b1))) if b0[k] != b1[k]), None))
    sb = (abi.Bytes * n)()
    for i in range(n):
        sb[i].data = C.addressof(out1) + scans[i].out_off
        sb[i].len = sb[i].cap = len1[i]
    glued = abi.Bytes()
    assert L.lep_file_recode_finish_progressive(f.handle, sb, n, C.byref(glued)) == 0
    data = glued.tobytes()
    L.lep_free(glued.data)
    assert data == jpg, (what, "the glued file is not the original")
    took = sum(t == LANE_RST for t in taken)
    if want_intervals:
        assert took > 0, (what, "no scan with an interval")
    markers = sum(sum(1 for k in range(len(b) - 1) if b[k] == 0xFF and 0xD0 <= b[k + 1] <= 0xD7) for (_, b, _, _), t in zip(res, taken) if t == LANE_RST)
    return took, markers


@pytest.mark.parametrize("name", ["prog_c422_rst_176x112", "androidprogressive", "iphoneprogressive2"])
def test_fixture_and_phone_images(core, lanes, name):
    """the fixture with restart intervals and the reference's two phone images (a DRI in front of every scan): every scan goes through the
    new form, byte for byte the wavefront form's; the glued file is the original"""
    jpg, lep = golden(name) if name.startswith("prog_") else ref_golden(name)
    took, markers = _three_assertions(core, lanes, jpg, lep, name)
    assert markers > 0
    print("%s: %d scans with an interval, %d markers through lep_huffprog_simt.h" % (name, took, markers))


def _pillow(w, h, mode, sub, quality, noise, seed, **restart):
    from PIL import Image, ImageFile

    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (max(2, h // 24), max(2, w // 24), 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(base, "RGB").resize((w, h), Image.BICUBIC)).astype(np.int16)
    a = np.clip(a + rng.normal(0, noise, a.shape), 0, 255).astype(np.uint8)
    kw = dict(format="JPEG", quality=quality, progressive=True, **restart)
    if mode == "RGB":
        kw["subsampling"] = sub
    buf = io.BytesIO()
    keep, ImageFile.MAXBLOCK = ImageFile.MAXBLOCK, max(ImageFile.MAXBLOCK, 1 << 22)   # (with its own guess of a buffer libjpeg gives up on some of these
    try:                                                                              # settings: "Suspension not allowed here")
        Image.fromarray(a, "RGB").convert(mode).save(buf, **kw)
    finally:
        ImageFile.MAXBLOCK = keep
    return buf.getvalue()


def _ac_table_without_end_of_band_code(jpg):
    """the test's own walk over the DHT segments: an AC table none of whose symbols is an EOBn code.  The planner leaves such a file to the
    host re-coder with or without restart intervals (jpeg_progressive.cc progressive_plan: "a table without any end-of-band code"), so it is
    no input for this sweep: tiny pictures at high quality come out that way, and the sweep draws them again at a lower quality."""
    pos = 2
    while pos + 4 <= len(jpg) and jpg[pos] == 0xFF and jpg[pos + 1] != 0xD9:
        kind, n = jpg[pos + 1], struct.unpack(">H", jpg[pos + 2:pos + 4])[0]
        if kind == 0xC4:
            p = pos + 4
            while p < pos + 2 + n:
                cnt = sum(jpg[p + 1:p + 17])
                if jpg[p] >> 4 and not any((sym & 15) == 0 and sym != 0xF0 for sym in jpg[p + 17:p + 17 + cnt]):
                    return True
                p += 17 + cnt
        pos += 2 + n
        if kind == 0xDA:
            while not (jpg[pos] == 0xFF and jpg[pos + 1] != 0 and not 0xD0 <= jpg[pos + 1] <= 0xD7):
                pos += 1
    return False


RESTARTS = [dict(restart_marker_blocks=b) for b in (1, 2, 3, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100, 516)] + [dict(restart_marker_rows=r) for r in (1, 2)]
LAYOUTS = [("L", 0), ("RGB", 0), ("RGB", 1), ("RGB", 2)]
# sizes: with and without padding blocks, a last interval that is short, components one block wide / one block high, scans shorter than the interval
SIZES = [(64, 48), (97, 72), (200, 150), (333, 241), (8, 200), (200, 8), (16, 16), (16, 120), (264, 16)]
QUALITIES, NOISES = [30, 75, 92, 100], [0, 2, 10, 40]


@pytest.mark.parametrize("restart", RESTARTS, ids=lambda r: "%s_%d" % next(iter(r.items())))
def test_generated_files(core, lanes, restart):
    """Pillow progressive files: every restart setting x every layout (grey, 4:4:4 / 4:2:2 / 4:2:0) x three sizes, which between them hold
    every size of the list for every setting.  restart_marker_blocks writes one DRI for the file (MCUs in the interleaved DC scan, blocks in
    the one-component scans), restart_marker_rows one per scan with an interval of its own: both routes into the scan's interval."""
    ri = RESTARTS.index(restart)
    files = took = markers = 0
    for li, (mode, sub) in enumerate(LAYOUTS):
        for k in range(3):
            w, h = SIZES[(3 * li + k + ri) % len(SIZES)]
            q, noise = QUALITIES[(k + li + ri) % 4], NOISES[(k + 2 * li + ri) % 4]
            jpg = _pillow(w, h, mode, sub, q, noise, 7000 + 64 * ri + 8 * li + k, **restart)
            for lower in (75, 30):
                if _ac_table_without_end_of_band_code(jpg):
                    q = lower
                    jpg = _pillow(w, h, mode, sub, q, noise, 7000 + 64 * ri + 8 * li + k, **restart)
            assert b"\xff\xdd" in jpg and not _ac_table_without_end_of_band_code(jpg)
            t, m = _three_assertions(core, lanes, jpg, None, (restart, mode, sub, w, h, q, noise))
            took += t; markers += m; files += 1
    assert files == 12
    if restart != dict(restart_marker_blocks=516):      # (longer than every scan of these sizes: a DRI and no marker)
        assert markers > 0
    print("%s: %d scans, %d markers" % (restart, took, markers))


def test_interval_longer_than_the_scan(core, lanes):
    """an interval of 516 in small pictures: every scan carries the interval, none a marker; the new form takes them all the same"""
    for mode, sub, w, h in [("L", 0, 97, 72), ("RGB", 2, 200, 150), ("RGB", 0, 64, 48)]:
        jpg = _pillow(w, h, mode, sub, 75, 10, 31, restart_marker_blocks=516)
        took, markers = _three_assertions(core, lanes, jpg, None, (mode, sub, w, h))
        assert took > 0 and markers == 0


def _drawn(rng, f, variant):
    """a frame drawn as coefficients (test_lane_per_unit_progressive_scan_encoder_on_drawn_frames' recipe)"""
    for c in range(f.desc.ncomp):
        nb = f.desc.nblocks(c)
        arr = np.zeros((nb, 64), dtype=np.int16)
        dens = [0.0, 0.02, 0.15, 0.6, 1.0][variant]
        mask = rng.random((nb, 64)) < dens
        vals = rng.integers(-40, 41, (nb, 64)).astype(np.int16)
        if variant == 3:
            vals = rng.integers(-2000, 2001, (nb, 64)).astype(np.int16)
        arr[mask] = vals[mask]
        if variant in (1, 2):   # whole stretches of blocks with nothing in them (end-of-band runs that reach and cross interval ends), and blocks that only hold old coefficients
            for _ in range(4):
                a = int(rng.integers(0, nb)); b = min(nb, a + int(rng.integers(1, max(2, nb // 2))))
                arr[a:b] = 0 if rng.random() < 0.5 else (arr[a:b] & ~1) * 2
        C.memmove(f.desc.blocks[c], arr.ctypes.data, nb * 128)


def _synth_plan(w, h, seed, sub, quality):
    from lepton_amd import corpus

    jpg = corpus.synth_jpeg(w, h, seed, progressive=True, subsampling=sub, quality=quality)
    return (jpg,) + _plan(jpg, None, (w, h, sub))


def test_drawn_frames(core, lanes):
    """the two forms on frames drawn as coefficients, with an interval set per scan: densities from empty to full, end-of-band runs that reach
    and cross interval ends, tables whose longest run is 1 / 3 / 7 / 31 blocks with intervals that are not multiples of it, a scan with
    interval 0 beside scans with intervals in one image, every pad-bit pattern"""
    rng = np.random.default_rng(78)
    intervals = [1, 2, 3, 5, 7, 8, 9, 31, 32, 33, 40, 63, 64, 65, 100, 1000]
    cases = with_markers = plain_beside = 0
    for trial, (w, h, sub) in enumerate([(160, 120, "4:2:0"), (203, 149, "4:4:4"), (8, 600, "4:2:0"), (700, 8, "4:2:2"), (333, 241, "4:2:0"), (96, 64, "4:2:2")]):
        jpg, f, img, scans, n = _synth_plan(w, h, 640 + trial, sub, [90, 60, 95, 30, 75, 85][trial])
        for variant in range(5):
            _drawn(rng, f, variant)
            for mx in (0, 1, 3, 7, 31):
                keep = [scans[i].max_eobrun for i in range(n)]
                img.padbit = [0, 1, 0x7f, 0xff, 0x55][(variant + trial) % 5]
                for i in range(n):
                    if mx and scans[i].to != 0:
                        scans[i].max_eobrun = min(mx, keep[i])
                    scans[i].rsti = int(rng.choice(intervals))
                zero = int(rng.integers(0, n))
                scans[zero].rsti = 0            # one scan without an interval beside the others
                res, taken, _ = _both_forms(core, lanes, img, scans, n)
                assert taken == [LANE if i == zero else LANE_RST for i in range(n)]
                plain_beside += 1
                outgrown = any(l0 & 0x80000000 for l0, _, _, _ in res) or sum(l0 for l0, _, _, _ in res) > len(jpg)
                for i, (l0, b0, l1, b1) in enumerate(res):
                    if l0 & 0x80000000:     # (a drawn frame may code to more than the file the plan was made for: both forms say so)
                        assert l1 & 0x80000000, (trial, variant, mx, i)
                        continue
                    if outgrown and (l1 & 0x80000000):   # (... and the scans behind it found the file's region used up)
                        continue
                    assert l0 == l1 and b0 == b1, (trial, variant, mx, i, scans[i].from_, scans[i].to, scans[i].sah, scans[i].sal, scans[i].rsti, l0, l1)
                    cases += 1
                    with_markers += i != zero and any(b0[k] == 0xFF and 0xD0 <= b0[k + 1] <= 0xD7 for k in range(len(b0) - 1))
                for i in range(n):
                    scans[i].max_eobrun = keep[i]
    assert cases > 500 and with_markers > 300 and plain_beside == 150, (cases, with_markers)


def test_region_that_does_not_suffice(core, lanes):
    """a region half the file's size: the scans left without a buffer answer "outgrew" (bit 31), the rest are still right, and nothing is
    written outside the region (the guard words _both_forms checks)"""
    jpg = _pillow(320, 240, "RGB", 2, 90, 10, 612, restart_marker_blocks=7)
    f, img, scans, n = _plan(jpg, None, "region")
    res, taken, _ = _both_forms(core, lanes, img, scans, n, region=len(jpg) // 2)
    assert all(t == LANE_RST for t in taken)
    assert any(l1 & 0x80000000 for _, _, l1, _ in res) and any(not (l1 & 0x80000000) for _, _, l1, _ in res)
    for l0, b0, l1, b1 in res:
        assert (l1 & 0x80000000) or (l0 == l1 and b0 == b1)
    # and with the new form off the same scans are the wavefront form's
    res, taken, _ = _both_forms(core, lanes, img, scans, n, rst_on=0)
    assert all(t == WAVE for t in taken) and all(l0 == l1 and b0 == b1 for l0, b0, l1, b1 in res)


def test_pad_bits_byte_boundaries_and_ff_in_front_of_a_marker(core, lanes):
    """a grey frame whose DC refinement scan codes one bit per block: with an interval of 8 / 16 blocks every interval ends exactly on a
    byte, with all bits set its bytes are FF -- stuffed, right in front of markers that are not; with intervals of 3 / 5 / 13 every interval
    is padded, by every pad-bit pattern"""
    from lepton_amd import corpus

    jpg = corpus.synth_jpeg(200, 152, 650, progressive=True, subsampling="4:4:4", quality=80)
    from PIL import Image
    buf = io.BytesIO()
    Image.open(io.BytesIO(jpg)).convert("L").save(buf, format="JPEG", quality=80, progressive=True)
    jpg = buf.getvalue()
    f, img, scans, n = _plan(jpg, None, "grey")
    refine = [i for i in range(n) if scans[i].to == 0 and scans[i].sah != 0]
    assert refine and all(scans[i].cmpc == 1 for i in range(n))
    nb = f.desc.nblocks(0)
    arr = np.zeros((nb, 64), dtype=np.int16)
    # all bits of the DC set: its refinement bit is 1 whatever the scan's Al.  Where the kernels keep the DC in a block is found, not assumed.
    dcpos = None
    seen_ff_marker = seen_pad = 0
    for at in range(64):
        arr[:] = 0
        arr[:, at] = -1
        C.memmove(f.desc.blocks[0], arr.ctypes.data, nb * 128)
        for i in range(n):
            scans[i].rsti = 8
        img.padbit = 0
        res, taken, _ = _both_forms(core, lanes, img, scans, n)
        b = res[refine[0]][1]
        if b.startswith(b"\xff\x00\xff\xd0\xff\x00\xff\xd1"):
            dcpos = at
            break
    assert dcpos is not None, "no coefficient position gives an all-ones DC refinement scan"
    for interval in (8, 16, 3, 5, 13):
        for pad in (0, 1, 0x7f, 0xff):
            for i in range(n):
                scans[i].rsti = interval
            img.padbit = pad
            res, taken, _ = _both_forms(core, lanes, img, scans, n)
            assert all(t == LANE_RST for t in taken)
            for i, (l0, b0, l1, b1) in enumerate(res):
                assert l0 < 0x80000000 and l0 == l1 and b0 == b1, (interval, pad, i)
            b = res[refine[0]][3]
            if interval % 8 == 0:
                unit = b"\xff\x00" * (interval // 8)
                assert b.startswith(unit + b"\xff\xd0" + unit + b"\xff\xd1"), b[:16]
                seen_ff_marker += 1
            else:
                bits = ((1 << interval) - 1) << (-interval % 8)
                fill = sum(((pad >> j) & 1) << (-interval % 8 - 1 - j) for j in range(-interval % 8))
                first = (bits | fill).to_bytes((interval + 7) // 8, "big").replace(b"\xff", b"\xff\x00")
                assert b.startswith(first + b"\xff\xd0"), (interval, pad, b[:8], first)
                seen_pad += 1
    assert seen_ff_marker == 8 and seen_pad == 12


def test_unit_map_is_a_closed_form(lanes):
    """the unit map against a plain walk: units of at most 32 blocks (8 MCUs) that never straddle an interval's end, in order, covering the scan"""
    lanes.emu_prog_rst_unit_map.restype = C.c_uint32
    lanes.emu_prog_rst_unit_map.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32]
    for mcus in (0, 1):
        per = 8 if mcus else 32
        for n in (1, 2, 7, 8, 9, 31, 32, 33, 64, 65, 100, 1000, 1023):
            for r in (1, 2, 3, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100, 516, 5000):
                want = []
                for b in range(0, n, r):
                    e = min(b + r, n)
                    want += [(a, min(a + per, e), b, e) for a in range(b, e, per)]
                spans = (C.c_uint32 * (4 * len(want) + 4))()
                assert lanes.emu_prog_rst_unit_map(n, r, mcus, spans, len(want)) == len(want), (mcus, n, r)
                assert [tuple(spans[4 * u: 4 * u + 4]) for u in range(len(want))] == want, (mcus, n, r)
            # a scan without an interval is a scan with one interval as long as the scan (or longer): units of `per` from the scan's first
            for r in (n, n + 1, n + per, 2 * n + 7):
                want = [(u * per, min((u + 1) * per, n), 0, n) for u in range((n + per - 1) // per)]
                spans = (C.c_uint32 * (4 * len(want) + 4))()
                assert lanes.emu_prog_rst_unit_map(n, r, mcus, spans, len(want)) == len(want), (mcus, n, r)
                assert [tuple(spans[4 * u: 4 * u + 4]) for u in range(len(want))] == want, (mcus, n, r)


def _place_made_up(lanes, nblocks, rsti, bits, region):
    n = len(bits)
    arr = (C.c_uint32 * n)(*bits)
    pos = (C.c_uint32 * n)()
    total, refused, buf_bytes, out_len = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    lanes.emu_prog_simt_rst_place_made_up.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    assert lanes.emu_prog_simt_rst_place_made_up(nblocks, rsti, arr, n, pos, C.byref(total), C.byref(refused), region, C.byref(buf_bytes), C.byref(out_len)) == 0
    return list(pos), total.value, refused.value, buf_bytes.value, out_len.value


def test_place_pass_sums_in_64_bits(lanes):
    """the place pass on made-up bit counts: positions are the serial walk's (pad to the byte and 16 marker bits behind every interval that
    ends inside the scan); a scan whose total passes 2^32 - 1 bits is refused -- no buffer, "outgrew" -- and one just under is not"""
    rng = np.random.default_rng(5)

    def serial(nblocks, rsti, bits):
        pos, at, u = [], 0, 0
        for b in range(0, nblocks, rsti):
            e = min(b + rsti, nblocks)
            for _ in range(b, e, 32):
                pos.append(at); at += bits[u]; u += 1
            if e < nblocks:
                at += (-at) % 8 + 16
        return pos, at

    for nblocks, rsti in [(1000, 33), (1000, 32), (4096, 100), (77, 1), (5000, 516), (64, 64)]:
        units = sum((min(b + rsti, nblocks) - b + 31) // 32 for b in range(0, nblocks, rsti))
        bits = [int(x) for x in rng.integers(0, 3000, units)]
        pos, total, refused, buf_bytes, _ = _place_made_up(lanes, nblocks, rsti, bits, 1 << 30)
        want_pos, want_total = serial(nblocks, rsti, bits)
        assert (pos, total, refused) == (want_pos, want_total, 0) and buf_bytes >= (total + 7) // 8
    # 70,000 units of 61,440 bits and a marker behind each: 2^32 is passed inside the scan
    nblocks, rsti = 70000 * 32, 32
    bits = [61440] * 70000
    _, total_exact = serial(nblocks, rsti, bits)
    assert total_exact > 0xffffffff
    pos, total, refused, buf_bytes, out_len = _place_made_up(lanes, nblocks, rsti, bits, 1 << 40)
    assert refused == 1 and buf_bytes == 0 and out_len == 0x80000000
    # the same bit counts on a scan without an interval: no markers, and 2^32 is still passed
    assert sum(bits) > 0xffffffff
    pos, total, refused, buf_bytes, out_len = _place_made_up(lanes, nblocks, 0, bits, 1 << 40)
    assert refused == 1 and buf_bytes == 0 and out_len & 0x80000000
    # ... and the scan with an interval cut short of it
    k = 0xffffffff // (61440 + 16) - 1
    pos, total, refused, buf_bytes, _ = _place_made_up(lanes, k * 32, rsti, bits[:k], 1 << 40)
    want_pos, want_total = serial(k * 32, rsti, bits[:k])
    assert refused == 0 and total == want_total and pos == want_pos and buf_bytes > 0


def _serial(units, at=0):
    """[(bits, interval ends here, marker written)] -> the units' positions and the total: pad to the byte and the marker's 16 behind an interval"""
    pos = []
    for bits, ends, marker in units:
        pos.append(at); at += bits
        if ends:
            at += (-at) % 8 + (16 if marker else 0)
    return pos, at


def _with_interval_sums(rng, lens, residues):
    """bit counts for intervals of lens[k] units whose sums are residues[k] modulo eight"""
    bits = []
    for n, r in zip(lens, residues):
        b = [int(x) for x in rng.integers(1, 3000, n)]
        b[-1] += (r - sum(b)) % 8
        bits += b
    return bits


def test_place_pass_pads_and_markers_of_both_writers(lanes):
    """the second stage of the place pass (simt_place_interval_extras) through both writers, on made-up bit counts against a prefix sum: intervals
    that end exactly on a byte (no pad bit) and one bit past one (seven); the sequential writer's first interval with 1..7 overhang bits in it,
    a segment that starts inside an interval, and rst_limit cutting the markers off half way"""
    rng = np.random.default_rng(11)
    # progressive, one-component scan: intervals of 70 blocks = 3 units (32, 32, 6), the last one short; every residue, 0 and 1 first
    nblocks, rsti = 70 * 9 + 40, 70
    lens = [3] * 9 + [2]
    for residues in ([0] * 10, [1] * 10, [0, 1, 7, 2, 0, 0, 1, 1, 5, 3]):
        bits = _with_interval_sums(rng, lens, residues)
        shape = [(b, k % 3 == 2 and k < 27, True) for k, b in enumerate(bits)]
        want_pos, want_total = _serial(shape)
        pos, total, refused, _, _ = _place_made_up(lanes, nblocks, rsti, bits, 1 << 30)
        assert (pos, total, refused) == (want_pos, want_total, 0), residues
        pads = [(-(sum(bits[3 * k: 3 * k + 3]))) % 8 for k in range(9)]
        assert pads == [(-r) % 8 for r in residues[:9]]
    # sequential: an image 5 MCUs wide and 40 high, intervals of 12 MCUs = 2 units (8, 4)
    lanes.emu_simt_enc_place_made_up.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    mcuh, mcuv, rsti = 5, 40, 12

    def sequential(row0, row1, overhang, rst_limit, residue_of):
        m, end, shape, k = row0 * mcuh, row1 * mcuh, [], 0
        while m < end:       # units of 8 MCUs that stop where an interval does
            stop = min(end, (m // rsti + 1) * rsti, m + 8)
            ends = stop % rsti == 0 and stop < mcuh * mcuv
            shape.append([int(rng.integers(1, 3000)), ends, ends and stop // rsti - 1 < rst_limit])
            if ends:         # the interval's bits (the first one's with the overhang bits) come to residue_of(k) modulo eight
                first = next((j + 1 for j in range(len(shape) - 2, -1, -1) if shape[j][1]), 0)
                have = sum(s[0] for s in shape[first:]) + (overhang if first == 0 else 0)
                shape[-1][0] += (residue_of(k) - have) % 8
                k += 1
            m = stop
        bits = (C.c_uint32 * len(shape))(*[s[0] for s in shape])
        pos, total = (C.c_uint32 * len(shape))(), C.c_uint32(0)
        assert lanes.emu_simt_enc_place_made_up(mcuh, mcuv, rsti, rst_limit, row0, row1, overhang, bits, len(shape), pos, C.byref(total)) == 0
        want_pos, want_total = _serial(shape, overhang)
        assert (list(pos), total.value) == (want_pos, want_total), (row0, row1, overhang, rst_limit)
        return sum(1 for s in shape if s[1]), sum(1 for s in shape if s[2])

    for overhang in range(8):
        for residue_of in (lambda k: 0, lambda k: 1, lambda k: (3 * k + 5) % 8):
            ends, markers = sequential(0, 40, overhang, 0xffffffff, residue_of)     # the whole scan: 16 intervals end inside it, none behind the last
            assert ends == markers == 16
            ends, markers = sequential(0, 40, overhang, 8, residue_of)              # markers cut off half way: pads go on, the 16 bits do not
            assert (ends, markers) == (16, 8)
            ends, markers = sequential(7, 23, overhang, 0xffffffff, residue_of)     # MCUs 35..114: starts 11 MCUs into an interval, ends 6 into one
            assert ends == markers == 7
            ends, markers = sequential(7, 23, overhang, 5, residue_of)              # ... with the limit falling inside the segment (markers 2, 3, 4 of 2..8)
            assert (ends, markers) == (7, 3)
