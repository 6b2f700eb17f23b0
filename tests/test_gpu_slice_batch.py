"""`-startbyte / -trunc` slices through the batch pipeline on the MI355X: lep_compress_batch_slices against lep_compress_slice (the
unchanged per-file host-path code: the yardstick), the 'Y' files it writes back through lep_decompress_batch on the lane scan
writer, and lep_huffdec_image.first_mcu_row on both scan decoders.  Files and positions: tests/slice_cases.py.  The lane decoder runs
with 1024-bit subsequences here (a codec object of the module's own, made while LEP_HUFFDEC_SIMT_BITS is set; the launch's name says what
it was cut with): shorter ones do not settle on files this small, which tests/test_slice_pipeline.py shows in the emulation."""
import ctypes as C
import os

import pytest

import slice_cases as sc
from lepton_amd import abi
from lepton_amd.codec import LeptonError

pytestmark = pytest.mark.gpu

SUB_BITS = 1024         # forced subsequence length of the lane decoder: a dozen and more lanes per file, lane boundaries inside MCU rows


def _extra_files():
    """layouts beyond tests/slice_cases.py that a slice now reaches the GPU parse path with (restart intervals: lane = interval; one
    component) and one the parser refuses (progressive)"""
    import numpy as np

    import jpeg_writer as jw
    from conftest import golden

    return {
        "rst": jw.write_baseline(96, 80, sc.LAYOUTS["420"][2], np.random.default_rng(77), restart_interval=3, density=0.05)[0],
        "gray": jw.write_baseline(64, 64, [(1, 1, 1, 0, 0, 0)], np.random.default_rng(78), density=0.05)[0],
        "prog": golden("prog_c420_320x240")[0],
    }


EXTRA = _extra_files()


def _jpg(name):
    return EXTRA[name] if name in EXTRA else sc.jpeg_of(name)


# 39 (file, slice) pairs of every kind of position -- whole files and refusals among them -- and a mid-scan slice of each further layout
PAIRS = [(l, s, t) for l in sc.LAYOUTS for s, t, _ in sc.positions(l)] + [("rst", len(EXTRA["rst"]) // 2, 0), ("gray", len(EXTRA["gray"]) // 2, 0),
                                                                             ("prog", 3000, 0)]


def _open_gpu(name, t):
    jpg = _jpg(name)
    n = min(len(jpg), t) if t else len(jpg)
    L = abi.lib()
    h, img, ok = C.c_void_p(), abi.HuffDecImage(), C.c_int(0)
    if L.lep_jpeg_open_gpu(jpg, n, C.byref(h), C.byref(img), C.byref(ok)):
        return None, None, False
    return h, img, bool(ok.value)


def _eligible(name, t):
    h, _, ok = _open_gpu(name, t)
    if h:
        abi.lib().lep_jpeg_close(h)
    return ok


def _decode_on_device(codec, name, fn_name, rows_to_try):
    """lep_gpu_huffman_decode{,_simt}_device on the whole file with first_mcu_row = each of rows_to_try: [(records, planes)], the image"""
    L = abi.lib()
    g = codec.handle
    h, img, ok = _open_gpu(name, 0)
    assert ok
    p, n = C.c_void_p(), C.c_size_t(0)
    L.lep_jpeg_scan_bytes(h, C.byref(p), C.byref(n))
    room = (n.value + 64 + 15) & ~15
    scan = C.string_at(p, n.value) + bytes(room - n.value)
    sizes = [img.bch[c] * img.vs[c] * img.mcuv * 128 for c in range(img.ncomp)]
    nrow = img.mcuv + 1
    d_scan, d_rows, d_planes = C.c_void_p(), C.c_void_p(), [C.c_void_p() for _ in sizes]
    assert L.lep_gpu_malloc(g, room, C.byref(d_scan)) == 0 and L.lep_gpu_malloc(g, nrow * C.sizeof(abi.HuffDecRow), C.byref(d_rows)) == 0
    for c, b in enumerate(sizes):
        assert L.lep_gpu_malloc(g, b, C.byref(d_planes[c])) == 0
        img.blocks[c] = d_planes[c].value
    out = []
    try:
        assert L.lep_gpu_memcpy_h2d(g, d_scan, scan, room) == 0
        img.scan, img.rows_off = d_scan.value, 0
        for r in rows_to_try:
            for c, b in enumerate(sizes):
                assert L.lep_gpu_memset(g, d_planes[c], 0, b) == 0
            assert L.lep_gpu_memset(g, d_rows, 0xEE, nrow * C.sizeof(abi.HuffDecRow)) == 0
            img.first_mcu_row = r
            assert getattr(L, fn_name)(g, C.byref(img), 1, d_rows, None) == 0 and L.lep_gpu_sync(g) == 0
            rows = (abi.HuffDecRow * nrow)()
            assert L.lep_gpu_memcpy_d2h(g, rows, d_rows, C.sizeof(rows)) == 0
            planes = []
            for c, b in enumerate(sizes):
                buf = C.create_string_buffer(b)
                assert L.lep_gpu_memcpy_d2h(g, buf, d_planes[c], b) == 0
                planes.append(buf.raw)
            out.append(([(x.bitpos, tuple(x.last_dc), x.aux) for x in rows], planes))
    finally:
        for d in [d_scan, d_rows] + d_planes:
            L.lep_gpu_free(g, d)
        L.lep_jpeg_close(h)
    return out, img


def _lane_launch(codec):
    """(lanes, bits per subsequence) of the codec's most recent lane-decoder launch, as the library names it"""
    import re

    m = re.search(r"\((\d+) lanes, (\d+) bits\)", abi.lib().lep_gpu_last_kernel_name(codec.handle).decode())
    assert m, "the lane-per-subsequence decoder did not take the launch"
    return int(m.group(1)), int(m.group(2))


@pytest.fixture(scope="module")
def codec():
    """a codec object of this module's own, made while LEP_HUFFDEC_SIMT_BITS is set: the variable is read when the object is made"""
    from lepton_amd.codec import GpuCodec

    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("LEP_HUFFDEC_SIMT_BITS", str(SUB_BITS))
        c = GpuCodec(0)
    # ... and it took: one scan through the lane decoder, cut into ceil(bits / 1024) lanes
    (_, img) = _decode_on_device(c, "420", "lep_gpu_huffman_decode_simt_device", [0])
    lanes, bits = _lane_launch(c)
    assert bits == SUB_BITS and lanes == (img.scan_len * 8 + SUB_BITS - 1) // SUB_BITS and lanes >= 10, (lanes, bits)
    yield c
    c.close()


@pytest.fixture(scope="module")
def yardstick(codec):
    """lep_compress_slice per pair, once: (status, .lep bytes or None)"""
    out = []
    for l, s, t in PAIRS:
        try:
            out.append((0, codec.compress_slice(_jpg(l), s, t)))
        except LeptonError as e:
            out.append((e.code, None))
    return out


def _scan_check_segments(name, s, t):
    """thread segments of the pair that `verify` writes again on the GPU: lep_jpeg_plan_scan_check's answer for the parsed slice"""
    L = abi.lib()
    jpg = _jpg(name)
    n = min(len(jpg), t) if t else len(jpg)
    h = C.c_void_p()
    if L.lep_jpeg_open_slice(jpg, n, s, C.byref(h)):
        return 0
    img, segs = abi.HuffImage(), (abi.HuffSegment * 16)()
    ff, fl, ns, ok = (C.c_uint32 * 16)(), (C.c_uint32 * 16)(), C.c_int(0), C.c_int(0)
    assert L.lep_jpeg_plan_scan_check(h, n, C.byref(img), segs, ff, fl, 16, C.byref(ns), C.byref(ok)) == 0
    L.lep_jpeg_close(h)
    return ns.value if ok.value else 0


@pytest.mark.parametrize("verify", [False, True])
def test_batch_slices_equal_the_per_file_call(codec, yardstick, verify):
    before = codec.scan_second_chances()
    leps, status, stats = codec.compress_batch([_jpg(l) for l, _, _ in PAIRS], verify=verify, slices=[(s, t) for _, s, t in PAIRS])
    assert status == [y[0] for y in yardstick]
    assert leps == [y[1] for y in yardstick]
    assert {0, 8, 14} <= set(status)                                # PROGRESSIVE_UNSUPPORTED and ONLY_GARBAGE_NO_JPEG among them
    # slices whose scan the GPU decoded: the pairs whose (bounded) file lep_jpeg_open_gpu calls eligible -- but for ONLY_GARBAGE_NO_JPEG,
    # which the host parser names after parsing that file again
    gpu = [_eligible(l, t) and y[0] != 14 for (l, s, t), y in zip(PAIRS, yardstick)]
    assert stats["gpu_huffman_files"] == sum(gpu) and sum(gpu) >= 30
    assert codec.scan_second_chances() == before                    # 1024-bit lanes settle on every one of these files
    if verify:
        assert stats["gpu_verified_scans"] == sum(_scan_check_segments(*p) for p, on in zip(PAIRS, gpu) if on)
        assert stats["gpu_verified_scans"] >= 15                    # per layout: whole, header, either side of a record, in front of the second row


def test_batch_decompress_writes_y_files_on_the_gpu(codec, yardstick):
    ys = [(p, y[1]) for p, y in zip(PAIRS, yardstick) if y[0] == 0 and y[1][3:4] == b"Y"]
    assert len(ys) >= 15                                            # per layout: header, either side of a record, in front of the second row, start + trunc inside the scan
    leps = [x for _, x in ys]
    want = [codec.decompress(x) for x in leps]
    assert want == [_jpg(l)[s:(t or None)] for (l, s, t), _ in ys]
    L = abi.lib()
    planned = 0
    for (l, s, t), x in ys:
        f = C.c_void_p()
        assert L.lep_file_open(x, len(x), C.byref(f)) == 0
        img, segs, nseg, ok = abi.HuffImage(), (abi.HuffSegment * 16)(), C.c_int(0), C.c_int(0)
        assert L.lep_file_recode_plan(f, C.byref(img), segs, C.byref(nseg), C.byref(ok)) == 0
        L.lep_file_close(f)
        cut_inside_scan = t != 0 and t < len(_jpg(l))
        assert ok.value == 1 or cut_inside_scan, (l, s, t)          # every 'Y' file of a whole scan is planned for the writer
        planned += ok.value
    out, status, stats = codec.decompress_batch(leps)
    assert status == [0] * len(leps) and out == want
    assert stats["gpu_huffman_files"] == planned                    # 'Y' files alone in the call: 0 on the commit before


def test_no_slices_is_the_whole_file_call(codec):
    import numpy as np

    import jpeg_writer as jw

    files = [jw.write_baseline(64 + 8 * k, 48 + 8 * (k % 3), sc.LAYOUTS[("420", "444", "422")[k % 3]][2], np.random.default_rng(900 + k), density=0.1)[0] for k in range(16)]
    a = codec.compress_batch(files)
    n = len(files)
    ins = (abi.Bytes * n)()
    keep = [C.create_string_buffer(f, len(f)) for f in files]
    for i, b in enumerate(keep):
        ins[i].data, ins[i].len, ins[i].cap = C.cast(b, C.c_void_p).value, len(files[i]), len(files[i])
    outs, status = (abi.Bytes * n)(), (C.c_int32 * n)()
    assert abi.lib().lep_compress_batch_slices(codec.handle, ins, None, n, outs, status, None, None) == 0
    got = [outs[i].tobytes() for i in range(n)]
    for i in range(n):
        abi.lib().lep_free(outs[i].data)
    assert list(status) == a[1] == [0] * n and got == a[0]


@pytest.mark.parametrize("layout", ["420", "422"])
def test_first_mcu_row_on_the_device(codec, layout):
    base = None
    for fn in ("lep_gpu_huffman_decode_simt_device", "lep_gpu_huffman_decode_device"):
        h, img0, _ = _open_gpu(layout, 0)
        abi.lib().lep_jpeg_close(h)
        tries = [0, 1, img0.mcuv // 2, img0.mcuv - 1, img0.mcuv]
        runs, img = _decode_on_device(codec, layout, fn, tries)
        if "simt" in fn:
            lanes, bits = _lane_launch(codec)
            assert bits == SUB_BITS and lanes == (img.scan_len * 8 + SUB_BITS - 1) // SUB_BITS and lanes >= 10   # lane boundaries every 1024 bits: inside MCU rows
        rec0, planes0 = runs[0]
        assert (rec0[img.mcuv][2] >> 8) == 0 and any(any(x) for x in planes0)
        if base is None:
            base = (rec0, planes0)
        assert (rec0, planes0) == base                              # the two decoders agree
        for r, (rec, planes) in zip(tries[1:], runs[1:]):
            assert rec == rec0, r
            for c in range(img.ncomp):
                cut = r * img.vs[c] * img.bch[c] * 128
                assert planes[c][cut:] == planes0[c][cut:] and not any(planes[c][:cut]), (r, c)
