"""What a launch function of lep_gpu.hip promises about the descriptor arrays it is given, on the MI355X: it keeps a copy of its own (the
pinned ring of staged blocks), so a caller may queue launch after launch without waiting -- more of them than the ring has slots -- and
may let its arrays go as soon as a call returns.  Through ctypes, like tests/test_gpu_pack_window.py; every call is a finite number of
launches and nothing is tried again."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden
from lepton_amd import abi
from test_gpu_pack import CANARY
from test_gpu_pack_window import window
from test_gpu_progressive_restart import _resident_scans
from test_gpu_progressive_restart_writer import _resident_frames
from test_pack_window_emulation import windows_of

pytestmark = pytest.mark.gpu

CALLS, RUNS, ROOM = 40, 3, 4096     # the ring has 16 slots


def _dmalloc(L, g, n):
    p = C.c_void_p()
    assert L.lep_gpu_malloc(g, max(n, 16), C.byref(p)) == 0
    return p


def test_forty_launches_without_a_wait(gpu_codec):
    """40 lep_gpu_pack_window_device calls on the codec's stream, nothing waited for between them: 3 runs each over a 4 KB source of the
    call's own, into a 4 KB destination of its own behind a canary; after ONE lep_gpu_sync every destination and every offset array is
    numpy's, and the bytes behind each total are the canary's"""
    L, g = gpu_codec._L, gpu_codec.handle
    rng = np.random.default_rng(26)
    src = rng.integers(0, 256, CALLS * ROOM, dtype=np.uint8)
    calls = []
    for k in range(CALLS):
        lens = [int(v) for v in rng.integers(0, 1301, RUNS)]
        offs = [int(rng.integers(0, ROOM - n + 1)) for n in lens]
        wins = [windows_of(n)[int(rng.integers(0, len(windows_of(n))))] for n in lens]
        calls.append((lens, offs, [s for s, _ in wins], [t for _, t in wins]))
    hlen = np.asarray([c[0] for c in calls], dtype=np.uint32)
    d_src, d_len, d_dst, d_off = _dmalloc(L, g, CALLS * ROOM), _dmalloc(L, g, hlen.nbytes), _dmalloc(L, g, CALLS * ROOM), _dmalloc(L, g, CALLS * (RUNS + 1) * 8)
    try:
        assert L.lep_gpu_memcpy_h2d(g, d_src, src.ctypes.data, src.nbytes) == 0 and L.lep_gpu_memcpy_h2d(g, d_len, hlen.ctypes.data, hlen.nbytes) == 0
        assert L.lep_gpu_memset(g, d_dst, CANARY, CALLS * ROOM) == 0 and L.lep_gpu_memset(g, d_off, 0xFF, CALLS * (RUNS + 1) * 8) == 0
        for k, (lens, offs, skips, takes) in enumerate(calls):
            so, sk, tk = (C.c_uint64 * RUNS)(*offs), (C.c_uint32 * RUNS)(*skips), (C.c_uint32 * RUNS)(*takes)
            rc = L.lep_gpu_pack_window_device(g, C.c_void_p(d_src.value + k * ROOM), so, C.c_void_p(d_len.value + k * RUNS * 4), sk, tk, RUNS,
                                              C.c_void_p(d_dst.value + k * ROOM), ROOM, C.c_void_p(d_off.value + k * (RUNS + 1) * 8), None)
            assert rc == 0, gpu_codec.last_error()
        assert L.lep_gpu_sync(g) == 0, gpu_codec.last_error()
        out, off = np.zeros(CALLS * ROOM, dtype=np.uint8), np.zeros(CALLS * (RUNS + 1), dtype=np.uint64)
        assert L.lep_gpu_memcpy_d2h(g, out.ctypes.data, d_dst, out.nbytes) == 0 and L.lep_gpu_memcpy_d2h(g, off.ctypes.data, d_off, off.nbytes) == 0
    finally:
        for p in (d_src, d_len, d_dst, d_off):
            L.lep_gpu_free(g, p)
    assert any(sum(window(n, s, t) for n, s, t in zip(c[0], c[2], c[3])) > 0 for c in calls)
    for k, (lens, offs, skips, takes) in enumerate(calls):
        wl = [window(n, s, t) for n, s, t in zip(lens, skips, takes)]
        total = sum(wl)
        mine, base = out[k * ROOM:(k + 1) * ROOM], k * ROOM
        want = np.concatenate([src[base + o + s:base + o + s + w] for o, s, w in zip(offs, skips, wl)])
        assert off[k * (RUNS + 1):(k + 1) * (RUNS + 1)].tolist() == [0] + np.cumsum(np.asarray(wl, dtype=np.uint64)).tolist(), k
        assert np.array_equal(mine[:total], want), (k, "bytes differ")
        assert (mine[total:] == CANARY).all(), (k, "bytes behind d_dst_off[n] were written")


def _wipe(array):
    C.memset(array, 0xFF, C.sizeof(array))


def _sequential_decode(codec, jpg, simt, wipe):
    """lep_gpu_huffman_decode_device / _simt_device on the file's scan resident on the device: (records, planes)"""
    from test_blind_wide_emulation import _open

    L, g = abi.lib(), codec.handle
    img, scan, planes, h = _open(jpg)
    if img.flags & 2:       # (LEP_HUFFDEC_RST_TABLE: the marker positions behind the scan bytes, as the flag promises)
        L.lep_jpeg_close(h)
        img, scan, planes, h = _open(jpg, with_restart_table=True)
    L.lep_jpeg_close(h)
    imgs = (abi.HuffDecImage * 1)()
    C.memmove(C.byref(imgs[0]), C.byref(img), C.sizeof(abi.HuffDecImage))
    sizes = [len(planes[c].raw) for c in range(img.ncomp)]
    nrows = img.mcuv + 1
    d_scan, d_frame, d_rows = _dmalloc(L, g, len(scan.raw)), _dmalloc(L, g, sum(sizes)), _dmalloc(L, g, nrows * C.sizeof(abi.HuffDecRow))
    try:
        assert L.lep_gpu_memcpy_h2d(g, d_scan, scan, len(scan.raw)) == 0
        assert L.lep_gpu_memset(g, d_frame, 0, sum(sizes)) == 0 and L.lep_gpu_memset(g, d_rows, 0, nrows * C.sizeof(abi.HuffDecRow)) == 0
        imgs[0].scan, imgs[0].rows_off, at = d_scan.value, 0, d_frame.value
        for c in range(img.ncomp):
            imgs[0].blocks[c] = at
            at += sizes[c]
        fn = L.lep_gpu_huffman_decode_simt_device if simt else L.lep_gpu_huffman_decode_device
        assert fn(g, imgs, 1, d_rows, None) == 0, codec.last_error()
        if wipe:
            _wipe(imgs)
        assert L.lep_gpu_sync(g) == 0, codec.last_error()
        frame, rows = C.create_string_buffer(sum(sizes)), (abi.HuffDecRow * nrows)()
        assert L.lep_gpu_memcpy_d2h(g, frame, d_frame, sum(sizes)) == 0 and L.lep_gpu_memcpy_d2h(g, rows, d_rows, nrows * C.sizeof(abi.HuffDecRow)) == 0
    finally:
        for p in (d_scan, d_frame, d_rows):
            L.lep_gpu_free(g, p)
    return [(r.bitpos, tuple(r.last_dc), r.aux) for r in rows], frame.raw


def _progressive_decode(codec, jpg, wipe):
    L, g = abi.lib(), codec.handle
    h, scans, n, d_frame, fbytes, d_rows, nrec, mem = _resident_scans(L, g, jpg)
    try:
        assert L.lep_gpu_huffman_progressive_decode_device(g, scans, n, d_rows, None) == 0, codec.last_error()
        if wipe:
            _wipe(scans)
        assert L.lep_gpu_sync(g) == 0, codec.last_error()
        frame, rows = C.create_string_buffer(fbytes), (abi.HuffDecRow * nrec)()
        assert L.lep_gpu_memcpy_d2h(g, frame, d_frame, fbytes) == 0 and L.lep_gpu_memcpy_d2h(g, rows, d_rows, nrec * C.sizeof(abi.HuffDecRow)) == 0
    finally:
        L.lep_jpeg_close(h)
        for m in mem:
            L.lep_gpu_free(g, m)
    return [(r.bitpos, tuple(r.last_dc), r.aux) for r in rows], frame.raw


def _progressive_encode(codec, jpg, wipe):
    """(byte count and bytes of every scan, the file's own bytes of every scan)"""
    L, g = abi.lib(), codec.handle
    imgs, scans, n, out_bytes, corr_words, mem, want = _resident_frames(L, g, [jpg])
    mem += [_dmalloc(L, g, out_bytes), _dmalloc(L, g, corr_words * 4), _dmalloc(L, g, n * 4 + 16)]
    d_out, d_corr, d_len = mem[-3:]
    try:
        out_off = [scans[i].out_off for i in range(n)]
        assert L.lep_gpu_memset(g, d_out, 0, out_bytes) == 0 and L.lep_gpu_memset(g, d_len, 0, n * 4 + 16) == 0
        assert L.lep_gpu_huffman_progressive_encode_device(g, imgs, 1, scans, n, d_out, d_corr, d_len, None) == 0, codec.last_error()
        if wipe:
            _wipe(imgs)
            _wipe(scans)
        assert L.lep_gpu_sync(g) == 0, codec.last_error()
        out, lens = C.create_string_buffer(out_bytes), (C.c_uint32 * n)()
        assert L.lep_gpu_memcpy_d2h(g, out, d_out, out_bytes) == 0 and L.lep_gpu_memcpy_d2h(g, lens, d_len, n * 4) == 0
    finally:
        for m in mem:
            L.lep_gpu_free(g, m)
    raw = out.raw
    return [(lens[i], raw[out_off[i]: out_off[i] + (lens[i] & 0x7fffffff)]) for i in range(n)], want


def test_descriptors_may_go_away_when_the_call_returns(gpu_codec):
    """each scan coder's device entry with the caller's descriptor arrays overwritten with 0xFF bytes the moment the call returns, before
    anything is waited for: rows, frames and scan bytes are those of the same sequence with the arrays left alone"""
    seq, prog = golden("q30_256x256_4seg")[0], golden("prog_c420_q97_800x600")[0]
    for simt in (False, True):       # the wavefront-per-file decoder, then the lane-per-subsequence one
        kept, wiped = _sequential_decode(gpu_codec, seq, simt, False), _sequential_decode(gpu_codec, seq, simt, True)
        assert any(r[0] for r in kept[0]) and any(kept[1]), "the decode left no record or no coefficient"
        assert wiped[0] == kept[0], (simt, "records differ")
        assert wiped[1] == kept[1], (simt, "frames differ")
    kept, wiped = _progressive_decode(gpu_codec, prog, False), _progressive_decode(gpu_codec, prog, True)
    assert any(r[0] for r in kept[0]) and any(kept[1]), "the progressive decode left no record or no coefficient"
    assert wiped[0] == kept[0], "progressive decode: records differ"
    assert wiped[1] == kept[1], "progressive decode: frames differ"
    (kept, want), (wiped, _) = _progressive_encode(gpu_codec, prog, False), _progressive_encode(gpu_codec, prog, True)
    assert [b for _, b in kept] == want, "progressive encode: not the file's own scan bytes"
    assert wiped == kept, "progressive encode: bytes differ"
