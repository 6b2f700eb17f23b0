"""lep_huffprogdec_rst.h -- progressive scans with restart intervals, one wavefront per piece of consecutive intervals -- as a lane-loop
emulation (tests/emu/prog_rst_emu.cc) against the host parser and against lep_huffprogdec.h, and the host side that feeds it: the marker
positions of every scan (lep_jpeg_scan_restarts_of) and the flag lep_jpeg_open_gpu_progressive sets on the scans that qualify."""
import ctypes as C
import io
import os
import random
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from conftest import golden, ref_golden, REF_GOLDEN  # noqa: E402
import test_core_emulation as tce  # noqa: E402

RST_TABLE = 2            # LEP_HUFFDEC_RST_TABLE
ONE_INTERVAL_PER_WAVE = 1
WHOLE_SCAN_IN_ONE_WAVE = 0xFFFFFFFF


def _build(src, so):
    tmp = "%s.%d" % (so, os.getpid())
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, src])
    os.replace(tmp, so)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def rst_emu():
    return _build(os.path.join(ROOT, "tests", "emu", "prog_rst_emu.cc"), os.path.join(ROOT, "tests", "emu", "libprog_rst_emu.so"))


@pytest.fixture(scope="module")
def core():
    """core_emu.cc as it is: emu_huffman_progressive_decode (lep_huffprogdec.h) is what the new form is held against"""
    return _build(os.path.join(ROOT, "tests", "emu", "core_emu.cc"), os.path.join(ROOT, "tests", "emu", "libcore_emu_progrst.so"))


def split_scans(jpg):
    """the test's own splitter: per SOS of the file (the DRI in force, length of the un-stuffed entropy-coded bytes, offsets in them at
    which a restart marker stood, whether every marker was the next of the D0..D7 cycle)"""
    out, pos, dri = [], 2, 0
    while pos + 4 <= len(jpg) and jpg[pos] == 0xFF and jpg[pos + 1] != 0xD9:
        kind, n = jpg[pos + 1], struct.unpack(">H", jpg[pos + 2:pos + 4])[0]
        if kind == 0xDD:
            dri = struct.unpack(">H", jpg[pos + 4:pos + 6])[0]
        pos += 2 + n
        if kind != 0xDA:
            continue
        length, marks, cyc = 0, [], True
        while pos + 1 < len(jpg):
            if jpg[pos] != 0xFF:
                length += 1; pos += 1
            elif jpg[pos + 1] == 0:
                length += 1; pos += 2
            elif 0xD0 <= jpg[pos + 1] <= 0xD7:
                cyc = cyc and jpg[pos + 1] == 0xD0 + (len(marks) & 7)
                marks.append(length); pos += 2
            else:
                break
        out.append((dri, length, marks, cyc))
    return out


def _units(sc):
    return sc.t.mcuc if sc.cmpc > 1 else sc.nch[sc.cmp[0]] * sc.ncv[sc.cmp[0]]


def _qualifies(sc, split):
    """a progressive scan with rsti > 0 that holds exactly the markers its length asks for, none of them at its very end"""
    dri, length, marks, cyc = split
    want = (_units(sc) - 1) // dri if dri > 0 else 0
    return (sc.from_, sc.to) != (0, 63) and dri > 0 and want > 0 and len(marks) == want and cyc and (not marks or marks[-1] < length)


def decode_rst(rst_emu, jpg, floor=0, info=None):
    """tce._progressive_decode_on_the_emulation for the new form: every flagged scan gets its marker positions behind its zero-padded slot
    (lep_jpeg_scan_restarts_of), the scans go through emu_huffman_progressive_decode_rst.  info receives taken / flagged / qualifies per
    scan, the records and the number of pieces."""
    from lepton_amd import abi

    L = abi.lib()
    L.lep_jpeg_scan_restarts_of.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_size_t)]
    h = C.c_void_p()
    plan1 = abi.HuffDecImage()
    ok = C.c_int(0)
    rc = L.lep_jpeg_open_gpu(jpg, len(jpg), C.byref(h), C.byref(plan1), C.byref(ok))
    assert rc == 0 and not ok.value, "a progressive file is not the sequential kernel's"
    scans = (abi.HuffProgDecScan * 64)()
    nscan, need, ok2 = C.c_int(0), C.c_int(0), C.c_int(0)
    assert L.lep_jpeg_open_gpu_progressive(h, scans, 64, C.byref(nscan), C.byref(need), C.byref(ok2)) == 0
    if not ok2.value:
        L.lep_jpeg_close(h)
        return None, None, None
    d = abi.ImageDesc()
    L.lep_jpeg_describe(h, C.byref(d))
    planes = [C.create_string_buffer(d.nblocks(c) * 128) for c in range(d.ncomp)]
    p, n = C.c_void_p(), C.c_size_t(0)
    L.lep_jpeg_scan_bytes(h, C.byref(p), C.byref(n))
    raw = C.string_at(p, n.value)
    split = split_scans(jpg)
    keep, flagged, qual = [], [], []
    for i in range(nscan.value):
        off, ln = scans[i].t.scan or 0, scans[i].t.scan_len
        room = (ln + 80 + 15) & ~15          # LEP_HUFFPROGDEC_SCAN_ROOM
        table = b""
        if scans[i].t.flags & RST_TABLE:
            rp, rn = C.POINTER(C.c_uint32)(), C.c_size_t(0)
            assert L.lep_jpeg_scan_restarts_of(h, i, C.byref(rp), C.byref(rn)) == 0
            table = struct.pack("<%dI" % rn.value, *rp[:rn.value])
        buf = C.create_string_buffer(raw[off:off + ln] + bytes(room - ln) + table, room + len(table) + 16)
        assert C.addressof(buf) % 16 == 0
        keep.append(buf)
        scans[i].t.scan = C.addressof(buf)
        for c in range(d.ncomp):
            scans[i].t.blocks[c] = C.addressof(planes[c])
        flagged.append(bool(scans[i].t.flags & RST_TABLE))
        qual.append(i < len(split) and _qualifies(scans[i], split[i]))
    rows = (abi.HuffDecRow * (need.value + 4))()
    taken = (C.c_int32 * 64)()
    pieces = C.c_uint32(0)
    again = C.c_int32(0)
    rst_emu.emu_huffman_progressive_decode_rst.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    assert rst_emu.emu_huffman_progressive_decode_rst(scans, nscan.value, rows, floor, taken, C.byref(pieces), C.byref(again)) == 0
    if info is not None:
        info.update(second_chance=bool(again.value), taken=[bool(taken[i]) for i in range(nscan.value)], flagged=flagged, qualifies=qual, pieces=pieces.value,
                    rows=[(r.bitpos, tuple(r.last_dc), r.aux) for r in rows])
    rc = L.lep_jpeg_finish_gpu_progressive(h, scans, nscan.value, rows)
    return h, planes, (0 if rc == 0 else -1)


def _three_equalities(rst_emu, core, jpg, what, floors=(0,), at_least=0):
    """the new form takes exactly the scans the splitter says qualify; planes and .lep header are the host parser's; every record is the one
    lep_huffprogdec.h (emu_huffman_progressive_decode) writes.  Returns how many scans the new form took."""
    from lepton_amd import abi

    rows_o = []
    h0, planes0, st0 = tce._progressive_decode_on_the_emulation(core, jpg, rows_out=rows_o)
    assert st0 == 0, (what, "lep_huffprogdec.h does not decode this file", st0)
    abi.lib().lep_jpeg_close(h0)
    took = 0
    for floor in floors:
        info = {}
        h, planes, st = decode_rst(rst_emu, jpg, floor, info)
        assert st == 0, (what, floor, "refused or found irregular", st, [r[2] >> 8 for r in info.get("rows", [])][-12:])
        assert not info["second_chance"], (what, floor, "an intact file must not need the older forms")
        assert info["taken"] == info["qualifies"] == info["flagged"], (what, floor, info["taken"], info["qualifies"], info["flagged"])
        took = sum(info["taken"])
        assert took >= at_least, (what, took)
        if floor == ONE_INTERVAL_PER_WAVE:
            assert info["pieces"] >= took
        if floor == WHOLE_SCAN_IN_ONE_WAVE:
            assert info["pieces"] == took
        tce._same_as_the_host_parser(jpg, h, planes)
        abi.lib().lep_jpeg_close(h)
        assert info["rows"] == rows_o, (what, floor, [i for i, (a, b) in enumerate(zip(info["rows"], rows_o)) if a != b][:8])
    return took


def _files_of_item_1():
    files = [("prog_c422_rst_176x112", golden("prog_c422_rst_176x112")[0])]
    files += [(n, ref_golden(n)[0]) for n in ("androidprogressive", "iphoneprogressive2")]
    return files


@pytest.mark.parametrize("name", ["prog_c422_rst_176x112", "androidprogressive", "iphoneprogressive2"])
def test_restart_interval_form_on_the_fixture_and_the_phone_images(rst_emu, core, name):
    """the fixture with restart intervals and the reference's two phone images (a DRI in front of every scan): at least one scan of each goes
    through the new form, every scan the splitter says qualifies does; planes, .lep header and records as before"""
    jpg = dict(_files_of_item_1())[name]
    took = _three_equalities(rst_emu, core, jpg, name, floors=(0, ONE_INTERVAL_PER_WAVE, WHOLE_SCAN_IN_ONE_WAVE), at_least=1)
    print("%s: %d of %d scans through lep_huffprogdec_rst.h" % (name, took, len(split_scans(jpg))))


def _pillow(w, h, mode, sub, quality, noise, seed, **restart):
    from PIL import Image

    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (max(2, h // 24), max(2, w // 24), 3), dtype=np.uint8)
    a = np.asarray(Image.fromarray(base, "RGB").resize((w, h), Image.BICUBIC)).astype(np.int16)
    a = np.clip(a + rng.normal(0, noise, a.shape), 0, 255).astype(np.uint8)
    kw = dict(format="JPEG", quality=quality, progressive=True, **restart)
    if mode == "RGB":
        kw["subsampling"] = sub
    buf = io.BytesIO()
    Image.fromarray(a, "RGB").convert(mode).save(buf, **kw)
    return buf.getvalue()


RESTARTS = [dict(restart_marker_blocks=b) for b in (1, 2, 3, 7, 8, 9, 63, 64, 65, 1000)] + [dict(restart_marker_rows=r) for r in (1, 3)]
LAYOUTS = [("L", 0), ("RGB", 0), ("RGB", 1), ("RGB", 2)]
WIDTHS, HEIGHTS, QUALITIES, NOISES = [64, 97, 200, 333], [48, 72, 150, 241], [30, 75, 92, 100], [0, 2, 10, 40]


@pytest.mark.parametrize("restart", RESTARTS, ids=lambda r: "%s_%d" % next(iter(r.items())))
def test_restart_interval_form_on_generated_files(rst_emu, core, restart):
    """Pillow progressive files: every restart setting x every layout (grey, 4:4:4 / 4:2:2 / 4:2:0) x four (size, quality, noise) draws that
    between them hold every width, height and quality of the grid -- sizes with and without padding blocks.  The piece floor forced to one
    interval per wave and to the whole scan in one wave.  No file is skipped and none may fall back."""
    ri = RESTARTS.index(restart)
    took = files = 0
    for li, (mode, sub) in enumerate(LAYOUTS):
        for k in range(4):
            w, h = WIDTHS[(k + li) % 4], HEIGHTS[(k + ri) % 4]
            q, noise = QUALITIES[(k + li + ri) % 4], NOISES[(k + 2 * li + ri) % 4]
            jpg = _pillow(w, h, mode, sub, q, noise, 3000 + 64 * ri + 8 * li + k, **restart)
            took += _three_equalities(rst_emu, core, jpg, (restart, mode, sub, w, h, q, noise), floors=(ONE_INTERVAL_PER_WAVE, WHOLE_SCAN_IN_ONE_WAVE))
            files += 1
    assert files == 16
    print("%s: %d scans of 16 files through lep_huffprogdec_rst.h" % (restart, took))
    if restart != dict(restart_marker_blocks=1000):
        assert took >= 16          # (an interval of 1000 blocks is longer than most scans of these sizes: those hold no marker)


def _chunks(jpg):
    """SOI | per scan: the segments in front of it, its SOS and its entropy-coded bytes | EOI"""
    out, pos, start = [], 2, 2
    while jpg[pos + 1] != 0xD9:
        kind, n = jpg[pos + 1], struct.unpack(">H", jpg[pos + 2:pos + 4])[0]
        pos += 2 + n
        if kind == 0xDA:
            while not (jpg[pos] == 0xFF and jpg[pos + 1] != 0 and not 0xD0 <= jpg[pos + 1] <= 0xD7):
                pos += 1
            out.append(jpg[start:pos]); start = pos
    return out


def test_restart_interval_form_beside_the_other_forms_in_one_file(rst_emu, core):
    """mixed routing.  (a) A progressive file in which ONE scan has DRI 0 -- that scan from the same picture written without restart markers, a
    DRI segment in front of it and behind it -- so one file takes the window form and the new one.  (b) Sequential frames coded in several
    scans with an interval per scan, 0 among them (tests/jpeg_writer.py): their scans are the sequential kernels', none is flagged."""
    import jpeg_writer as jw

    for sub, k in [(2, 3), (0, 5), (1, 9)]:
        with_rst = _pillow(200, 150, "RGB", sub, 75, 10, 41 + sub, restart_marker_blocks=7)
        without = _pillow(200, 150, "RGB", sub, 75, 10, 41 + sub)
        a, b = _chunks(with_rst), _chunks(without)
        assert len(a) == len(b) == 10
        dri = lambda v: b"\xff\xdd" + struct.pack(">HH", 4, v)
        jpg = b"\xff\xd8" + b"".join(a[:k]) + dri(0) + b[k] + dri(7) + b"".join(a[k + 1:]) + b"\xff\xd9"
        info = {}
        took = _three_equalities(rst_emu, core, jpg, ("spliced", sub, k), floors=(0, ONE_INTERVAL_PER_WAVE, WHOLE_SCAN_IN_ONE_WAVE), at_least=9)
        assert took == 9
        h, planes, st = decode_rst(rst_emu, jpg, 0, info)
        assert st == 0 and info["taken"] == [i != k for i in range(10)]
        from lepton_amd import abi
        abi.lib().lep_jpeg_close(h)
    for name, intervals in [("y_cbcr_420", [12, 0]), ("y_cb_cr_444", [0, 7, 3]), ("cbcr_y_420", [4, 0]), ("two_y_c", [1, 0])]:
        comps, scans = tce.SEQUENTIAL_SCAN_SCRIPTS[name]
        for w, h in [(97, 50), (333, 250)]:
            jpg, _ = jw.write_sequential_scans(w, h, comps, np.random.default_rng(zlib.crc32(("rst %s %d" % (name, w)).encode())), scans, restart_intervals=intervals, density=0.3)
            assert _three_equalities(rst_emu, core, jpg, (name, w, h), floors=(ONE_INTERVAL_PER_WAVE, WHOLE_SCAN_IN_ONE_WAVE)) == 0


def _seeds_with_restart_intervals():
    seeds = [golden("prog_c422_rst_176x112")[0]]
    seeds += [_pillow(97, 72, "RGB", 2, 75, 10, 501, restart_marker_blocks=3), _pillow(200, 48, "L", 0, 92, 2, 502, restart_marker_rows=1),
              _pillow(64, 150, "RGB", 0, 30, 40, 503, restart_marker_blocks=8), _pillow(97, 48, "RGB", 1, 75, 10, 504, restart_marker_blocks=1)]
    assert all(len(s) < 30000 for s in seeds)
    return seeds


def _old_form(core, j):
    from lepton_amd import abi

    rows = []
    try:
        h, planes, st = tce._progressive_decode_on_the_emulation(core, j, rows_out=rows)
    except AssertionError:
        return None
    if st is not None:
        abi.lib().lep_jpeg_close(h)
    return (st, [p.raw for p in planes] if st == 0 else None, rows if st == 0 else None)


def _new_form(rst_emu, j, floor, info):
    from lepton_amd import abi

    try:
        h, planes, st = decode_rst(rst_emu, j, floor, info)
    except AssertionError:
        return None
    if st is not None:
        abi.lib().lep_jpeg_close(h)
    return (st, [p.raw for p in planes] if st == 0 else None, info["rows"] if st == 0 else None)


def test_restart_interval_form_on_damaged_files(rst_emu, core):
    """220 files with restart intervals damaged inside their scans and in their headers (test_core_emulation's recipe, a seed of its own):
    the new form asks for the host parser on exactly the files lep_huffprogdec.h asks for it; where both decode, frames and records are
    equal; a scan whose markers no longer count up to what its length asks for is not flagged and never reaches the new form.
    An interval of a damaged file that does not end at its marker sets a status in the new form, yet the reference -- which never looks at
    where the markers stood -- may decode on from there: such a file gets lep_huffprogdec.h as a second chance, as in the batch pipeline.
    The floors: lep_huffprogdec.h alone yields both = 63, refused = 99 on this seed (the rest is not a progressive file any more, or not
    eligible); the test asks for four fifths of each, the slack the existing test leaves itself."""
    rnd = random.Random(1907)
    seeds = _seeds_with_restart_intervals()
    both = refused = unflagged = reached = 0
    for trial in range(220):
        j, kind = tce._mutated_progressive(rnd, seeds)
        old = _old_form(core, j)
        info = {}
        new = _new_form(rst_emu, j, (0, ONE_INTERVAL_PER_WAVE, WHOLE_SCAN_IN_ONE_WAVE)[trial % 3], info)
        if old is None or new is None:
            assert old is None and new is None, (trial, kind)
            continue
        assert old[0] == new[0], (trial, kind, old[0], new[0])
        if "taken" in info:
            assert info["taken"] == info["flagged"]
            reached += sum(info["taken"])
            for f, q in zip(info["flagged"], info["qualifies"]):
                assert not (f and not q), (trial, kind, "a scan whose markers do not count up is flagged")
                unflagged += (not f)
        if old[0] == 0:
            assert old[1] == new[1] and old[2] == new[2], (trial, kind)
            both += 1
        elif old[0] == -1:
            refused += 1
    assert both >= 50 and refused >= 80 and reached > 100, "both %d refused %d (lep_huffprogdec.h alone on this seed: 63 / 99); scans through the new form %d" % (both, refused, reached)
    print("both %d refused %d; scans through the new form %d, left un-flagged %d" % (both, refused, reached, unflagged))
    # the last marker of the first scan deleted, and one more added behind it: the scan is left un-flagged, the other scans are not
    seed = seeds[1]
    sos2 = seed.find(b"\xff\xda", seed.find(b"\xff\xda") + 2)
    at = [i for i in range(seed.find(b"\xff\xda"), sos2) if seed[i] == 0xFF and 0xD0 <= seed[i + 1] <= 0xD7]
    assert len(at) > 5
    last = at[-1]
    for j in (seed[:last] + seed[last + 2:], seed[:last + 3] + b"\xff" + bytes([0xD0 + (seed[last + 1] - 0xD0 + 1) % 8]) + seed[last + 3:]):
        old, info = _old_form(core, j), {}
        new = _new_form(rst_emu, j, 0, info)
        assert old is not None and new is not None and old[0] == new[0]
        assert info["flagged"][0] is False and info["taken"][0] is False and any(info["flagged"][1:]), info["flagged"]


def test_marker_positions_of_every_scan(rst_emu):
    """lep_jpeg_scan_restarts_of: scan 0 as lep_jpeg_scan_restarts; (units - 1) / rsti positions per scan; every position the offset in the
    un-stuffed scan at which the file really had a marker (the test's own splitter)"""
    from lepton_amd import abi

    L = abi.lib()
    L.lep_jpeg_scan_restarts_of.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_size_t)]
    files = _files_of_item_1() + [("pillow %d" % i, s) for i, s in enumerate(_seeds_with_restart_intervals()[1:])]
    files.append(("no markers", _pillow(97, 72, "RGB", 2, 75, 10, 7)))
    for name, jpg in files:
        h, plan1, ok = C.c_void_p(), abi.HuffDecImage(), C.c_int(0)
        assert L.lep_jpeg_open_gpu(jpg, len(jpg), C.byref(h), C.byref(plan1), C.byref(ok)) == 0
        scans = (abi.HuffProgDecScan * 64)()
        nscan, need, ok2 = C.c_int(0), C.c_int(0), C.c_int(0)
        assert L.lep_jpeg_open_gpu_progressive(h, scans, 64, C.byref(nscan), C.byref(need), C.byref(ok2)) == 0 and ok2.value
        split = split_scans(jpg)
        assert len(split) == nscan.value
        rp, rn = C.POINTER(C.c_uint32)(), C.c_size_t(0)
        for i, (dri, length, marks, cyc) in enumerate(split):
            assert L.lep_jpeg_scan_restarts_of(h, i, C.byref(rp), C.byref(rn)) == 0
            got = rp[:rn.value]
            assert scans[i].t.rsti == dri and scans[i].t.scan_len == length
            assert rn.value == ((_units(scans[i]) - 1) // dri if dri else 0), (name, i)
            assert got == marks and all(0 < p < length for p in got), (name, i)
            assert bool(scans[i].t.flags & RST_TABLE) == (rn.value > 0)
            if i == 0:
                p0, n0 = C.POINTER(C.c_uint32)(), C.c_size_t(0)
                L.lep_jpeg_scan_restarts.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_size_t)]
                L.lep_jpeg_scan_restarts(h, C.byref(p0), C.byref(n0))
                assert p0[:n0.value] == got
        assert L.lep_jpeg_scan_restarts_of(h, nscan.value, C.byref(rp), C.byref(rn)) != 0 and L.lep_jpeg_scan_restarts_of(h, -1, C.byref(rp), C.byref(rn)) != 0
        L.lep_jpeg_close(h)
