"""Progressive files that END INSIDE A SCAN on the scan kernels, stepped on the CPU (tests/emu/prog_cut_emu.cc over prog_cut_driver.h).

Compress direction: the window decoder (lep_huffprogdec_win.h) with LEP_HUFFDEC_EARLY_EOF on the file's last scan + lep_jpeg_finish_gpu_progressive
must leave the host parser's frame and the host parser's container, byte for byte, for every cut the host parser accepts; it may decline
(a status, the file goes to the host parser) only where lep_jpeg_cut_block_irregular says the block that met the end had failed to decode.
Decompress direction: from the .lep so made, the lane scan writer (lep_huffprog_simt.h) + lep_file_recode_finish_progressive must restore
the cut file, with the plan saying gpu_ok and no scan flagged as outgrown.

Inputs: byte cuts jpg[:p] of three whole fixtures (the sweeps below, a cut right behind every scan's last data byte, 1 and 2 bytes into the
marker that follows) and the five prog_truncated_* fixtures.  Every slot's room is 0xFF in the driver: the bits behind the data's last are
zeros by position, not by what the slot holds."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from conftest import golden  # noqa: E402
import oracle_binding as ob  # noqa: E402
import test_core_emulation as tce  # noqa: E402

EARLY_EOF = 1                 # LEP_HUFFDEC_EARLY_EOF
ROW_TRUNCATED = 0x40000000    # LEP_HUFFDEC_ROW_TRUNCATED

# file -> (first cut, stride); "sos + 14": 14 bytes behind the first FF DA
SWEEPS = {"prog_c420_320x240": ("sos+14", 97), "prog_c444_203x149": (700, 61), "prog_gray_120x88": (400, 23)}
REGULAR = ["prog_truncated_dc", "prog_truncated_mid", "prog_truncated_q97_800x600", "prog_truncated_tail"]
IRREGULAR = "prog_truncated_refine_overrun"


@pytest.fixture(scope="module")
def cut_emu():
    src = os.path.join(ROOT, "tests", "emu", "prog_cut_emu.cc")
    so = os.path.join(ROOT, "tests", "emu", "libprog_cut_emu.so")
    tmp = "%s.%d" % (so, os.getpid())
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, src])
    os.replace(tmp, so)
    return C.CDLL(so)


def scan_spans(jpg):
    """per SOS of the file: (offset of the first entropy-coded byte, offset of the marker that ends the scan)"""
    out, pos = [], 2
    while pos + 4 <= len(jpg) and jpg[pos] == 0xFF and jpg[pos + 1] != 0xD9:
        kind, n = jpg[pos + 1], (jpg[pos + 2] << 8) | jpg[pos + 3]
        pos += 2 + n
        if kind != 0xDA:
            continue
        first = pos
        while pos + 1 < len(jpg) and not (jpg[pos] == 0xFF and jpg[pos + 1] != 0 and not 0xD0 <= jpg[pos + 1] <= 0xD7):
            pos += 1
        out.append((first, pos))
    return out


def sweep_cuts(name):
    jpg = golden(name)[0]
    first, stride = SWEEPS[name]
    if first == "sos+14":
        first = jpg.index(b"\xff\xda") + 14
    cuts = set(range(first, len(jpg) - 2, stride))         # up to len - 3
    for _, end in scan_spans(jpg):
        cuts.update(p for p in (end, end + 1, end + 2) if p <= len(jpg) - 3)
    return jpg, sorted(cuts)


def host_parse(jpg):
    """(rc, irregular, JpegImage or None) of the host parser"""
    from lepton_amd import abi
    from lepton_amd.codec import JpegImage, LeptonError

    try:
        img = JpegImage(jpg)
    except LeptonError as e:
        return e.code, 0, None
    return 0, abi.lib().lep_jpeg_cut_block_irregular(img.handle), img


def decode_on_the_emulation(cut_emu, jpg, win=True, pipelined=False, misalign=False, info=None):
    """(handle, planes, status): status None = not eligible, -1 = declined (a status in a record / finish refused), 0 = finished"""
    from lepton_amd import abi

    L = abi.lib()
    h = C.c_void_p()
    plan1 = abi.HuffDecImage()
    ok = C.c_int(0)
    rc = L.lep_jpeg_open_gpu(jpg, len(jpg), C.byref(h), C.byref(plan1), C.byref(ok))
    assert rc == 0 and not ok.value
    scans = (abi.HuffProgDecScan * 64)()
    nscan, need, ok2 = C.c_int(0), C.c_int(0), C.c_int(0)
    assert L.lep_jpeg_open_gpu_progressive_cut(h, scans, 64, C.byref(nscan), C.byref(need), C.byref(ok2)) == 0
    if not ok2.value:
        L.lep_jpeg_close(h)
        return None, None, None
    n = nscan.value
    flags = [scans[i].t.flags & EARLY_EOF for i in range(n)]
    assert flags == [0] * (n - 1) + [EARLY_EOF], ("the last descriptor alone carries the flag", flags)
    assert all(scans[i].t.rsti == 0 for i in range(n))
    d = abi.ImageDesc()
    L.lep_jpeg_describe(h, C.byref(d))
    planes = [C.create_string_buffer(d.nblocks(c) * 128) for c in range(d.ncomp)]
    p, ln = C.c_void_p(), C.c_size_t(0)
    L.lep_jpeg_scan_bytes(h, C.byref(p), C.byref(ln))
    raw = C.string_at(p, ln.value)
    for i in range(n):
        for c in range(d.ncomp):
            scans[i].t.blocks[c] = C.addressof(planes[c])
    rows = (abi.HuffDecRow * (need.value + 4))()
    taken, declined = C.c_int32(0), C.c_int32(0)
    cut_emu.emu_prog_cut_decode_file.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert cut_emu.emu_prog_cut_decode_file(scans, n, raw, len(raw), int(win), int(pipelined), int(misalign), rows, C.byref(taken), C.byref(declined)) == 0
    if info is not None:
        fin = rows[scans[n - 1].result_off]
        info.update(nscan=n, taken=taken.value, declined=declined.value, final=(fin.bitpos, tuple(fin.last_dc), fin.aux))
    rc = L.lep_jpeg_finish_gpu_progressive(h, scans, n, rows)
    return h, planes, (0 if rc == 0 else -1)


def lep_of(img):
    return img.write_lep(ob.oracle_encode(img.desc, img.plan())[0])


def write_on_the_emulation(cut_emu, jpg, lep, frame_of, info=None):
    """the cut file restored from `lep` with its scans written by the lane writer from the frame `frame_of` holds (a JpegImage)"""
    from lepton_amd import abi
    from lepton_amd.codec import LepFile

    L = abi.lib()
    f = LepFile(lep)
    for c in range(f.desc.ncomp):
        C.memmove(f.desc.blocks[c], frame_of.desc.blocks[c], f.desc.nblocks(c) * 128)
    img = abi.HuffProgImage()
    scans = (abi.HuffProgScan * 64)()
    nscan, ok = C.c_int(0), C.c_int(0)
    assert L.lep_file_recode_plan_progressive_cut(f.handle, C.byref(img), scans, 64, C.byref(nscan), C.byref(ok)) == 0
    assert ok.value, "gpu_ok: the plan takes a file cut inside a scan"
    n = nscan.value
    out_total = corr_total = 0
    for i in range(n):
        scans[i].image = 0
        scans[i].out_off = out_total
        out_total += (scans[i].out_cap + 15) & ~15
        scans[i].corr_off = corr_total
        corr_total += scans[i].corr_cap
    out = C.create_string_buffer(out_total + 64)
    corr = (C.c_uint32 * (corr_total + 8))()
    lens = (C.c_uint32 * n)()
    taken = (C.c_int32 * n)()
    guards = C.c_int32(0)
    coded = (C.c_int32 * 4)(*[f.desc.coded_blocks[c] if c < f.desc.ncomp else 0 for c in range(4)])
    cut_emu.emu_prog_cut_write_file.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    assert cut_emu.emu_prog_cut_write_file(C.byref(img), scans, n, len(f.segments), coded, out, corr, lens, taken, C.byref(guards)) == 0
    assert guards.value == 1, "the writer wrote outside its region or unit arrays"
    assert all(l < 0x80000000 for l in lens), ("a scan outgrew its slot", [hex(l) for l in lens])
    assert all(t == 1 for t in taken), ("the lane writer takes every scan", list(taken))
    if info is not None:
        info.update(nsegs=len(f.segments), lens=list(lens), coded=list(coded), all_blocks=[f.desc.nblocks(c) for c in range(f.desc.ncomp)],
                    scans=[out.raw[scans[i].out_off:scans[i].out_off + lens[i]] for i in range(n)])
    sb = (abi.Bytes * n)()
    for i in range(n):
        sb[i].data = C.addressof(out) + scans[i].out_off
        sb[i].len = sb[i].cap = lens[i]
    res = abi.Bytes()
    assert L.lep_file_recode_finish_progressive(f.handle, sb, n, C.byref(res)) == 0
    data = res.tobytes()
    L.lep_free(res.data)
    return data


def both_directions(cut_emu, jpg, what, want_lep=None, **kw):
    """Returns "refused" (the host parser's rc != 0), "declined" (allowed where the getter says irregular) or "ok"."""
    from lepton_amd import abi

    rc, irregular, host = host_parse(jpg)
    if rc:
        return "refused"
    info = {}
    h, planes, status = decode_on_the_emulation(cut_emu, jpg, info=info, **kw)
    assert status is not None, (what, "eligible: lep_jpeg_open_gpu_progressive_cut takes a progressive file cut inside a scan")
    try:
        if status != 0:
            assert irregular, (what, "declined a cut whose final block decoded", info)
            return "declined"
        assert info["taken"] == info["nscan"] and info["declined"] == 0, (what, info)
        tce._same_as_the_host_parser(jpg, h, planes)
    finally:
        abi.lib().lep_jpeg_close(h)
    lep = lep_of(host)
    if want_lep is not None:
        assert lep == want_lep, (what, "not the committed .lep")
    assert write_on_the_emulation(cut_emu, jpg, lep, host) == jpg, (what, "the lane writer does not restore the cut file")
    return "ok"


@pytest.mark.parametrize("name", sorted(SWEEPS))
def test_sweep_of_cuts_both_directions(cut_emu, name):
    jpg, cuts = sweep_cuts(name)
    spans = scan_spans(jpg)
    accepted = []
    for p in cuts:                                            # the test's own input first: no accepted cut is irregular ...
        rc, irregular, _ = host_parse(jpg[:p])
        if rc == 0:
            assert irregular == 0, (name, p, "an irregular cut in the sweep: the kernels may decline it, the sweep must say so")
            accepted.append(p)
    for k, (first, end) in enumerate(spans):                  # ... and every scan of the file holds one
        assert any(first < p <= end for p in accepted), (name, "no accepted cut inside scan", k, first, end)
    assert len(accepted) >= 80, (name, len(accepted))
    for p in accepted:
        assert both_directions(cut_emu, jpg[:p], (name, p)) == "ok", (name, p)


@pytest.mark.parametrize("pipelined", [False, True])
def test_the_five_fixtures(cut_emu, pipelined):
    for name in REGULAR:
        jpg, lep = golden(name)
        assert both_directions(cut_emu, jpg, name, want_lep=lep, pipelined=pipelined) == "ok", name
    jpg, _ = golden(IRREGULAR)
    rc, irregular, _ = host_parse(jpg)
    assert rc == 0 and irregular == 1, "prog_truncated_refine_overrun is the irregular kind by construction"
    assert both_directions(cut_emu, jpg, IRREGULAR, pipelined=pipelined) == "declined"


def test_whole_files_say_regular():
    for name in sorted(SWEEPS):
        assert host_parse(golden(name)[0])[:2] == (0, 0)


def test_a_cut_scan_no_kernel_knows_goes_to_none(cut_emu):
    """the window form switched off, or the cut scan's slot not aligned (prog_win_takes): the plan sends the flagged scan to no kernel, its
    record says not written, finish refuses -- the older form must never see the flag"""
    jpg = golden("prog_truncated_mid")[0]
    for kw in (dict(win=False), dict(misalign=True)):
        info = {}
        h, planes, status = decode_on_the_emulation(cut_emu, jpg, info=info, **kw)
        assert status == -1 and info["declined"] == 1 and info["final"][2] < 0, (kw, info)
        from lepton_amd import abi
        abi.lib().lep_jpeg_close(h)


def test_several_thread_segments(cut_emu):
    """prog_truncated_q97_800x600 is coded as several thread segments: the writer reads the frame as it is"""
    jpg, lep = golden("prog_truncated_q97_800x600")
    _, _, host = host_parse(jpg)
    info = {}
    assert write_on_the_emulation(cut_emu, jpg, lep, host, info=info) == jpg
    assert info["nsegs"] > 1, info


def test_lazy_tail_of_a_single_segment_file(cut_emu):
    """a file of ONE thread segment whose stream codes a first block of a row behind trunc_bc: the reference's re-coder reads zeros there.
    The frame handed to the writer is the DECODER's view -- the host parser's frame with such a block set to what the stream could code --
    so the test fails if the clear in front of the scan launch is missing."""
    from lepton_amd.codec import LepFile

    found = None
    for name in sorted(SWEEPS):
        jpg, cuts = sweep_cuts(name)
        for p in cuts:
            rc, _, host = host_parse(jpg[:p])
            if rc:
                continue
            f = LepFile(lep_of(host))
            d = f.desc
            if len(f.segments) != 1:
                continue
            # a component whose cut stands inside a block row that is not its last: the first block of the next row lies behind trunc_bc
            for c in range(d.ncomp):
                row_end = (d.coded_blocks[c] + d.width_blocks[c] - 1) // d.width_blocks[c] * d.width_blocks[c]
                if d.coded_blocks[c] < row_end < d.nblocks(c):
                    found = (name, p, c, row_end)
                    break
            if found:
                break
        if found:
            break
    assert found, "no sweep cut of one thread segment leaves a row's first block behind trunc_bc: construct one from prog_truncated_dc"
    name, p, c, row_end = found
    jpg = golden(name)[0][:p]
    _, _, host = host_parse(jpg)
    lep = lep_of(host)
    # the scans as written from the host parser's frame (zero behind the cut) ...
    clean = {}
    assert write_on_the_emulation(cut_emu, jpg, lep, host, info=clean) == jpg, found
    assert clean["nsegs"] == 1
    # ... and from the DECODER's view of it: what a decoder that takes every row's first block leaves there is anything but zero (DC in
    # aligned order: index 49, as the kernels store it).  The bytes behind the cut are nobody's, so the whole scans are held, not the file
    blk = (C.c_int16 * 64).from_address(host.desc.blocks[c] + row_end * 128)
    assert not any(blk), "the host parser leaves the block behind the cut zero"
    blk[49] = 64
    seen = {}
    assert write_on_the_emulation(cut_emu, jpg, lep, host, info=seen) == jpg, found
    assert seen["scans"] == clean["scans"], "the writer read a block behind trunc_bc of a single-segment file"
