"""Progressive files with restart intervals WRITTEN on the MI355X: lep_huffprog_simt.h (one lane per run of blocks, units cut at the
intervals' ends) through the batch decompressor, the round-trip check of the batch compressor and the device entry, against the original
files and against the same build with LEP_HUFFPROG_SIMT_RST=0 (the wavefront form, lep_huffprog.h).  Every call is a finite number of
launches; nothing is tried again after a failure."""
import ctypes as C
import io
import os

import numpy as np
import pytest

from conftest import golden, golden_cases, ref_golden
from lepton_amd import abi
from lepton_amd.codec import GpuCodec, JpegImage, LepFile

pytestmark = pytest.mark.gpu

LANE, LANE_RST, WAVE, SEQ = 0, 1, 2, 3


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


def _codec(**env):
    """a codec made with the given knobs (they are read when the codec is made)"""
    for k, v in env.items():
        os.environ[k] = v
    try:
        return GpuCodec(0)
    finally:
        for k in env:
            del os.environ[k]


def _forms(codec):
    counts = (C.c_uint32 * 4)()
    assert abi.lib().lep_gpu_huffman_progressive_encode_forms(codec.handle, C.byref(counts)) == 0
    return list(counts)


def _planner_takes(lep):
    f = LepFile(lep)
    img, scans = abi.HuffProgImage(), (abi.HuffProgScan * 64)()
    n, ok = C.c_int(0), C.c_int(0)
    assert abi.lib().lep_file_recode_plan_progressive(f.handle, C.byref(img), scans, 64, C.byref(n), C.byref(ok)) == 0
    return bool(ok.value)


@pytest.fixture(scope="module")
def files():
    """(with intervals, without): [(name, jpg, lep)].  The generated files' .lep is what the build answers with the new form off."""
    off = _codec(LEP_HUFFPROG_SIMT_RST="0")
    with_rst = [("prog_c422_rst_176x112",) + golden("prog_c422_rst_176x112")]
    with_rst += [(n,) + ref_golden(n) for n in ("androidprogressive", "iphoneprogressive2")]
    for name, w, h, seed, restart in [("1080p_rows_1", 1920, 1080, 21, dict(restart_marker_rows=1)), ("1080p_blocks_5", 1920, 1080, 22, dict(restart_marker_blocks=5)),
                                      ("4k_rows_1", 3840, 2160, 23, dict(restart_marker_rows=1)), ("4k_blocks_5", 3840, 2160, 24, dict(restart_marker_blocks=5))]:
        j = restart_jpeg(w, h, seed, **restart)
        with_rst.append((name, j, off.compress(j)))
    off.close()
    without = [(n,) + golden(n) for n in golden_cases() if n.startswith("prog_") and n != "prog_c422_rst_176x112"]
    assert all(_planner_takes(l) for _, _, l in with_rst)
    return with_rst, without


def _decompress_three_times(codec, files, want_rst_form):
    with_rst, without = files
    both = without + with_rst          # (the files with intervals last: the batch's last launch is the write of their scans)
    leps, jpgs = [l for _, _, l in both], [j for _, j, _ in both]
    takes = sum(_planner_takes(l) for l in leps)
    assert takes >= len(with_rst) + 3
    for chunk_images in (0, 2, 0):          # (2: chunks of two images, which overlap in the pipeline)
        back, st, stats = codec.decompress_batch(leps, chunk_images=chunk_images)
        assert st == [0] * len(leps), st
        assert [b == j for b, j in zip(back, jpgs)] == [True] * len(leps)
        assert stats["gpu_huffman_files"] == takes, stats
        if want_rst_form:                   # (with the new form off the last chunk holds wavefront-form scans only)
            assert "huffprog_simt" in abi.lib().lep_gpu_last_kernel_name(codec.handle).decode()
    # the files with intervals alone, in one chunk: which form wrote their scans
    back, st, stats = codec.decompress_batch([l for _, _, l in with_rst])
    assert st == [0] * len(with_rst) and back == [j for _, j, _ in with_rst] and stats["gpu_huffman_files"] == len(with_rst)
    forms = _forms(codec)
    if want_rst_form:
        assert forms[LANE_RST] > 0 and forms[WAVE] == 0 and forms[SEQ] == 0, forms
        assert "huffprog_simt" in abi.lib().lep_gpu_last_kernel_name(codec.handle).decode()
    else:
        assert forms[LANE_RST] == 0 and forms[WAVE] > 0, forms
    return forms


def test_decompress_batch_writes_restart_interval_scans_with_the_lane_form(files):
    """the fixture with restart intervals, the reference's two phone images, 1080p and 4K files with a marker per MCU row and per five
    blocks, and the progressive fixtures without intervals in one batch, three times (once in chunks of two images): statuses 0, the
    original files, every file the planner takes written on the GPU, no scan of a file with intervals left to the wavefront form"""
    codec = GpuCodec(0)
    try:
        forms = _decompress_three_times(codec, files, True)
        print("scans by form (lane, lane with intervals, wavefront, sequential):", forms)
    finally:
        codec.close()


def test_decompress_batch_with_the_new_form_off(files):
    """LEP_HUFFPROG_SIMT_RST=0: the same bytes, the scans with intervals from the wavefront form"""
    codec = _codec(LEP_HUFFPROG_SIMT_RST="0")
    try:
        _decompress_three_times(codec, files, False)
    finally:
        codec.close()


def test_round_trip_check_of_the_batch_compressor(files):
    """compress_batch(verify=True) of the files with intervals: the goldens' bytes (generated files: what the build answers with the new
    form off), no file done again by the host"""
    with_rst, _ = files
    codec = GpuCodec(0)
    try:
        for _ in range(2):
            got, st, stats = codec.compress_batch([j for _, j, _ in with_rst], verify=True)
            assert st == [0] * len(with_rst)
            assert [g == l for g, (_, _, l) in zip(got, with_rst)] == [True] * len(with_rst)
            assert stats["redone_files"] == 0, stats
        forms = _forms(codec)
        assert forms[LANE_RST] > 0 and forms[WAVE] == 0, forms
    finally:
        codec.close()


def _resident_frames(L, g, jpgs):
    """the files' frames resident on the device and the plan that writes every scan again (lep_jpeg_plan_progressive_check): (images, scans,
    n, output arena bytes, correction-bit dwords, what to free)"""
    imgs, all_scans, mem = [], [], []
    out_total = corr_total = 0
    for k, jpg in enumerate(jpgs):
        src = JpegImage(jpg)
        img, scans = abi.HuffProgImage(), (abi.HuffProgScan * 64)()
        first, flen = (C.c_uint32 * 64)(), (C.c_uint32 * 64)()
        n, ok = C.c_int(0), C.c_int(0)
        assert L.lep_jpeg_plan_progressive_check(src.handle, len(jpg), C.byref(img), scans, first, flen, 64, C.byref(n), C.byref(ok)) == 0 and ok.value
        for c in range(src.desc.ncomp):
            nbytes = src.desc.nblocks(c) * 128
            d = C.c_void_p()
            assert L.lep_gpu_malloc(g, nbytes, C.byref(d)) == 0
            assert L.lep_gpu_memcpy_h2d(g, d, C.string_at(src.desc.blocks[c], nbytes), nbytes) == 0
            img.blocks[c] = d.value
            mem.append(d)
        imgs.append(img)
        for i in range(n.value):
            sc = abi.HuffProgScan.from_buffer_copy(scans[i])
            sc.image = k
            sc.out_cap = min(sc.out_cap, flen[i] + 64)
            sc.out_off = out_total
            out_total += (sc.out_cap + 15) & ~15
            sc.corr_off = corr_total
            corr_total += sc.corr_cap
            all_scans.append((sc, jpg[first[i]: first[i] + flen[i]]))
    return (abi.HuffProgImage * len(imgs))(*imgs), (abi.HuffProgScan * len(all_scans))(*[s for s, _ in all_scans]), len(all_scans), out_total + 64, corr_total + 8, mem, [w for _, w in all_scans]


@pytest.mark.parametrize("which", ["prog_c422_rst_176x112", "androidprogressive", "iphoneprogressive2", "1080p_rows_1", "1080p_blocks_5", "4k_rows_1", "mixed"])
def test_device_entry_with_the_new_form_on_and_off(files, which):
    """lep_gpu_huffman_progressive_encode_device on resident frames: out_len and bytes of every scan equal with LEP_HUFFPROG_SIMT_RST on and
    off, and equal to the file's own bytes of that scan; `mixed`: images with and without intervals in one launch"""
    with_rst, without = files
    by_name = {n: j for n, j, _ in with_rst + without}
    jpgs = [by_name[which]] if which != "mixed" else [by_name["prog_c422_rst_176x112"], by_name["prog_c420_320x240"], by_name["1080p_blocks_5"], by_name["androidprogressive"]]
    L = abi.lib()
    results = []
    for env in ({}, {"LEP_HUFFPROG_SIMT_RST": "0"}):
        codec = _codec(**env)
        try:
            g = codec.handle
            imgs, scans, n, out_bytes, corr_words, mem, want = _resident_frames(L, g, jpgs)
            d_out, d_corr, d_len = C.c_void_p(), C.c_void_p(), C.c_void_p()
            assert L.lep_gpu_malloc(g, out_bytes, C.byref(d_out)) == 0 and L.lep_gpu_malloc(g, corr_words * 4, C.byref(d_corr)) == 0 and L.lep_gpu_malloc(g, n * 4 + 16, C.byref(d_len)) == 0
            assert L.lep_gpu_memset(g, d_out, 0, out_bytes) == 0 and L.lep_gpu_memset(g, d_len, 0, n * 4 + 16) == 0
            assert L.lep_gpu_huffman_progressive_encode_device(g, imgs, len(jpgs), scans, n, d_out, d_corr, d_len, None) == 0, codec.last_error()
            assert L.lep_gpu_sync(g) == 0, codec.last_error()
            name, forms = L.lep_gpu_last_kernel_name(g).decode(), _forms(codec)
            out, lens = C.create_string_buffer(out_bytes), (C.c_uint32 * n)()
            assert L.lep_gpu_memcpy_d2h(g, out, d_out, out_bytes) == 0 and L.lep_gpu_memcpy_d2h(g, lens, d_len, n * 4) == 0
            for m in mem + [d_out, d_corr, d_len]:
                L.lep_gpu_free(g, m)
            raw = out.raw
            results.append((name, forms, list(lens), [raw[scans[i].out_off: scans[i].out_off + (lens[i] & 0x7fffffff)] for i in range(n)], want))
        finally:
            codec.close()
    (name_on, forms_on, lens_on, bytes_on, want), (name_off, forms_off, lens_off, bytes_off, _) = results
    assert forms_on[LANE_RST] > 0 and forms_on[WAVE] == 0 and "huffprog_simt" in name_on, (forms_on, name_on)
    assert forms_off[LANE_RST] == 0 and forms_off[WAVE] == forms_on[LANE_RST] and forms_off[LANE] == forms_on[LANE], (forms_on, forms_off)
    assert lens_on == lens_off and all(l < 0x80000000 for l in lens_on)
    assert bytes_on == bytes_off, [i for i, (a, b) in enumerate(zip(bytes_on, bytes_off)) if a != b]
    assert bytes_on == want, [i for i, (a, b) in enumerate(zip(bytes_on, want)) if a != b]
