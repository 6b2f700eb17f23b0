"""Progressive files with restart intervals on the MI355X: lep_huffprogdec_rst.h (one wavefront per piece of consecutive intervals) through
the batch compressor and through the device entry, against the committed goldens and against the same build with LEP_HUFFPROGDEC_RST=0
(lep_huffprogdec.h).  Every call is a finite number of launches; nothing is tried again after a failure."""
import ctypes as C
import io
import os
import struct

import numpy as np
import pytest

from conftest import golden, golden_cases, ref_golden
from lepton_amd import abi
from lepton_amd.codec import GpuCodec, LeptonError

pytestmark = pytest.mark.gpu

RST_TABLE = 2


def restart_jpeg(w, h, seed, **restart):
    """a Pillow progressive file (4:2:0, quality 90) of a smooth picture with texture, restart markers as asked"""
    from PIL import Image

    rng = np.random.default_rng(seed)
    base = Image.fromarray(rng.integers(0, 256, (max(2, h // 64), max(2, w // 64), 3), dtype=np.uint8), "RGB").resize((w, h), Image.BICUBIC)
    tex = Image.fromarray(rng.integers(0, 48, (max(2, h // 4), max(2, w // 4), 3), dtype=np.uint8), "RGB").resize((w, h), Image.BILINEAR)
    a = np.clip(np.asarray(base, dtype=np.int16) + np.asarray(tex, dtype=np.int16) - 24, 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(a, "RGB").save(buf, format="JPEG", quality=90, subsampling=2, progressive=True, **restart)
    return buf.getvalue()


@pytest.fixture(scope="module")
def generated():
    return [restart_jpeg(1920, 1080, 11, restart_marker_rows=1), restart_jpeg(1920, 1080, 12, restart_marker_blocks=5),
            restart_jpeg(3840, 2160, 13, restart_marker_rows=1), restart_jpeg(3840, 2160, 14, restart_marker_blocks=5)]


@pytest.fixture(scope="module")
def without_the_new_form(generated):
    """what the same build answers with LEP_HUFFPROGDEC_RST=0 (the knob is read when the codec is made)"""
    os.environ["LEP_HUFFPROGDEC_RST"] = "0"
    try:
        codec = GpuCodec(0)
    finally:
        del os.environ["LEP_HUFFPROGDEC_RST"]
    want = [codec.compress(j) for j in generated]
    yield codec, want
    codec.close()


def test_batch_of_restart_interval_files_three_times(generated, without_the_new_form):
    """the reference's two phone images, the fixture with restart intervals, 1080p and 4K files with a marker per MCU row and per five
    blocks, and the progressive fixtures without restart intervals, in one batch -- three times, a level-ordering mistake would not show
    every time: statuses 0, the goldens' bytes (generated files: what the build answers with the new form off), every file's scans
    decoded on the GPU, no scan gave up waiting"""
    _, want_generated = without_the_new_form
    names = [n for n in golden_cases() if n.startswith("prog_")]
    assert "prog_c422_rst_176x112" in names
    jpgs = [golden(n)[0] for n in names]
    leps = [golden(n)[1] for n in names]
    for n in ("androidprogressive", "iphoneprogressive2"):
        j, l = ref_golden(n)
        jpgs.append(j); leps.append(l)
    jpgs += generated; leps += want_generated
    codec = GpuCodec(0)
    for _ in range(3):
        got, st, stats = codec.compress_batch(jpgs)
        assert st == [0] * len(jpgs)
        assert [g == l for g, l in zip(got, leps)] == [True] * len(jpgs)
        # (every file's scans are decoded on the GPU -- but for the fixtures cut inside their scans, which are the host parser's by design)
        assert stats["gpu_huffman_files"] == len(jpgs) - sum("truncated" in n for n in names)
    assert abi.lib().lep_jpeg_gpu_scan_wait_timeouts() == 0
    codec.close()


def _resident_scans(L, g, jpg, clear_flag=False):
    """the file's scans resident on the device as the batch pipeline lays them out (slot, marker positions behind it), a zeroed frame, a
    record arena; returns (host handle, descriptors, n, frame pointer, frame bytes, rows pointer, records, everything to free)"""
    h, plan1, ok = C.c_void_p(), abi.HuffDecImage(), C.c_int(0)
    assert L.lep_jpeg_open_gpu(jpg, len(jpg), C.byref(h), C.byref(plan1), C.byref(ok)) == 0 and not ok.value
    scans = (abi.HuffProgDecScan * 64)()
    nscan, need, ok2 = C.c_int(0), C.c_int(0), C.c_int(0)
    assert L.lep_jpeg_open_gpu_progressive(h, scans, 64, C.byref(nscan), C.byref(need), C.byref(ok2)) == 0 and ok2.value
    p, n = C.c_void_p(), C.c_size_t(0)
    L.lep_jpeg_scan_bytes(h, C.byref(p), C.byref(n))
    raw = C.string_at(p, n.value)
    arena, offs = bytearray(), []
    for i in range(nscan.value):
        off, ln = scans[i].t.scan or 0, scans[i].t.scan_len
        room = (ln + 80 + 15) & ~15
        offs.append(len(arena))
        arena += raw[off:off + ln] + bytes(room - ln)
        if scans[i].t.flags & RST_TABLE:
            rp, rn = C.POINTER(C.c_uint32)(), C.c_size_t(0)
            assert L.lep_jpeg_scan_restarts_of(h, i, C.byref(rp), C.byref(rn)) == 0 and rn.value > 0
            arena += struct.pack("<%dI" % rn.value, *rp[:rn.value])
            arena += bytes(-len(arena) % 16)
    arena += bytes(256)
    sizes = [scans[0].t.bch[c] * scans[0].bcv[c] * 128 for c in range(scans[0].t.ncomp)]
    d_scan, d_frame, d_rows = C.c_void_p(), C.c_void_p(), C.c_void_p()
    nrec = need.value + 4
    assert L.lep_gpu_malloc(g, len(arena), C.byref(d_scan)) == 0 and L.lep_gpu_malloc(g, sum(sizes), C.byref(d_frame)) == 0
    assert L.lep_gpu_malloc(g, nrec * C.sizeof(abi.HuffDecRow), C.byref(d_rows)) == 0
    assert d_scan.value % 16 == 0
    assert L.lep_gpu_memcpy_h2d(g, d_scan, bytes(arena), len(arena)) == 0
    assert L.lep_gpu_memset(g, d_frame, 0, sum(sizes)) == 0 and L.lep_gpu_memset(g, d_rows, 0, nrec * C.sizeof(abi.HuffDecRow)) == 0
    for i in range(nscan.value):
        scans[i].t.scan = d_scan.value + offs[i]
        at = d_frame.value
        for c in range(scans[0].t.ncomp):
            scans[i].t.blocks[c] = at
            at += sizes[c]
        if clear_flag:
            scans[i].t.flags &= ~RST_TABLE
    return h, scans, nscan.value, d_frame, sum(sizes), d_rows, nrec, (d_scan, d_frame, d_rows)


@pytest.mark.parametrize("which", ["prog_c422_rst_176x112", "androidprogressive", "iphoneprogressive2", "1080p_rows", "1080p_blocks_5", "4k_rows"])
def test_device_entry_with_the_new_form_on_and_off(generated, without_the_new_form, which):
    """lep_gpu_huffman_progressive_decode_device on resident scans: frames and every record equal with LEP_HUFFPROGDEC_RST on and off (and
    with the flag cleared by the caller); the kernel's name says which form ran"""
    off_codec, _ = without_the_new_form
    jpg = {"1080p_rows": generated[0], "1080p_blocks_5": generated[1], "4k_rows": generated[2]}.get(which)
    if jpg is None:
        jpg = golden(which)[0] if which.startswith("prog_") else ref_golden(which)[0]
    L = abi.lib()
    on_codec = GpuCodec(0)
    results = []
    for codec, clear in ((on_codec, False), (off_codec, False), (on_codec, True)):
        g = codec.handle
        h, scans, n, d_frame, fbytes, d_rows, nrec, mem = _resident_scans(L, g, jpg, clear_flag=clear)
        assert any(scans[i].t.flags & RST_TABLE for i in range(n)) != clear
        assert L.lep_gpu_huffman_progressive_decode_device(g, scans, n, d_rows, None) == 0, codec.last_error()
        assert L.lep_gpu_sync(g) == 0, codec.last_error()
        name = L.lep_gpu_last_kernel_name(g).decode()
        frame, rows = C.create_string_buffer(fbytes), (abi.HuffDecRow * nrec)()
        assert L.lep_gpu_memcpy_d2h(g, frame, d_frame, fbytes) == 0 and L.lep_gpu_memcpy_d2h(g, rows, d_rows, nrec * C.sizeof(abi.HuffDecRow)) == 0
        assert L.lep_jpeg_finish_gpu_progressive(h, scans, n, rows) == 0
        L.lep_jpeg_close(h)
        for m in mem:
            L.lep_gpu_free(g, m)
        results.append((name, frame.raw, [(r.bitpos, tuple(r.last_dc), r.aux) for r in rows]))
    on_codec.close()
    assert "huffprogdec_rst" in results[0][0] and "huffprogdec_rst" not in results[1][0] and "huffprogdec_rst" not in results[2][0], [r[0] for r in results]
    assert results[0][1] == results[1][1] == results[2][1], "frames differ"
    assert results[0][2] == results[1][2] == results[2][2], "records differ"


def test_device_entry_with_a_mixed_launch():
    """ONE call of lep_gpu_huffman_progressive_decode_device holding the scans of three files, interleaved file by file: the fixture with
    restart intervals (the interval form), a progressive fixture without (the pipelined launch) and a sequential frame in two scans (the
    lane decoder) -- every part of the launch plan (lep_scan_decode_plan.h) at once, row_off / result_off shifted per file as the batch
    pipeline shifts them.  Frames and every record equal what three separate calls give; the kernel's name is the last part's."""
    L = abi.lib()
    codec = GpuCodec(0)
    g = codec.handle
    names = ["prog_c422_rst_176x112", "prog_c420_320x240", "seq_ycb_cr_422_640x480_2seg"]
    files = [_resident_scans(L, g, golden(n)[0]) for n in names]
    nrow = C.sizeof(abi.HuffDecRow)

    def frames_and_records(d_rows_of, first_of):
        out = []
        for k, (h, scans, n, d_frame, fbytes, d_rows, nrec, mem) in enumerate(files):
            frame, rows = C.create_string_buffer(fbytes), (abi.HuffDecRow * nrec)()
            assert L.lep_gpu_memcpy_d2h(g, frame, d_frame, fbytes) == 0
            assert L.lep_gpu_memcpy_d2h(g, rows, C.c_void_p(d_rows_of(k).value + first_of(k) * nrow), nrec * nrow) == 0
            out.append((frame.raw, [(r.bitpos, tuple(r.last_dc), r.aux) for r in rows]))
        return out

    for h, scans, n, d_frame, fbytes, d_rows, nrec, mem in files:                      # three separate calls
        assert L.lep_gpu_huffman_progressive_decode_device(g, scans, n, d_rows, None) == 0, codec.last_error()
        assert L.lep_gpu_sync(g) == 0, codec.last_error()
    want = frames_and_records(lambda k: files[k][5], lambda k: 0)
    assert any(f[1][i][0] for f in want for i in range(len(f[1]))), "the separate calls left no record"
    # one call: the frames wiped, one record arena, file k's records from first[k] on
    first = [sum(f[6] for f in files[:k]) for k in range(3)]
    total = sum(f[6] for f in files)
    d_all = C.c_void_p()
    assert L.lep_gpu_malloc(g, total * nrow, C.byref(d_all)) == 0 and L.lep_gpu_memset(g, d_all, 0, total * nrow) == 0
    mixed = (abi.HuffProgDecScan * sum(f[2] for f in files))()
    at = 0
    for i in range(max(f[2] for f in files)):
        for k, (h, scans, n, d_frame, fbytes, d_rows, nrec, mem) in enumerate(files):
            if i >= n:
                continue
            C.memmove(C.byref(mixed[at]), C.byref(scans[i]), C.sizeof(abi.HuffProgDecScan))
            mixed[at].t.rows_off += first[k]
            mixed[at].result_off += first[k]
            at += 1
    assert at == len(mixed)
    for h, scans, n, d_frame, fbytes, d_rows, nrec, mem in files:
        assert L.lep_gpu_memset(g, d_frame, 0, fbytes) == 0
    assert L.lep_gpu_huffman_progressive_decode_device(g, mixed, at, d_all, None) == 0, codec.last_error()
    assert L.lep_gpu_sync(g) == 0, codec.last_error()
    name = L.lep_gpu_last_kernel_name(g).decode()
    got = frames_and_records(lambda k: d_all, lambda k: first[k])
    for h, scans, n, d_frame, fbytes, d_rows, nrec, mem in files:
        L.lep_jpeg_close(h)
        for m in mem:
            L.lep_gpu_free(g, m)
    L.lep_gpu_free(g, d_all)
    codec.close()
    assert "huffprogdec_rst" in name, name
    for k, n in enumerate(names):
        assert got[k][0] == want[k][0], (n, "frames differ")
        assert got[k][1] == want[k][1], (n, "records differ")


def test_damaged_big_files_with_restart_intervals(generated):
    """three damaged 1080p files (inside different scans): status and bytes as per-file compress gives them"""
    codec = GpuCodec(0)
    big = generated[0]
    bad = []
    for k in (3, 5, 7):
        b = bytearray(big); b[len(b) * k // 9] ^= 0x24
        bad.append(bytes(b))
    want = []
    for b in bad:
        try:
            want.append((0, codec.compress(b)))
        except LeptonError as e:
            want.append((e.code, None))
    want_big = codec.compress(big)
    got, st, _ = codec.compress_batch(bad + [big, generated[1]])
    assert st[3:] == [0, 0] and got[3] == want_big
    for (code, w), s, g_ in zip(want, st[:3], got[:3]):
        assert (s, g_) == (code, w) or (code == 41 and s == 0)   # per-file compress also runs the round-trip check
    codec.close()
