"""The resumable decoder on the GPU: lep_gpu_decode_rows_begin / _advance / _end (lep_decode_v4_rows_kernel) and lep_decompress_stream.

A launch of several files is advanced band by band; after every advance the frames (device buffers that started filled with 0x5a) are read
back and held against the oracle's frame: every block row a record reports as done has its final content, every other block row of the
segment still holds the fill, a segment that finished stays as it is while its neighbours go on.  Damaged streams must stop at the block
the oracle stops at.  A session owns its workspace set, and lep_decompress_stream hands out lep_decompress's bytes in pieces.

How many advances a launch takes: a band moves EVERY running segment on by band_mcu_rows MCU rows (each stops in front of the MCU row it
resumed in + band), so a launch is over after ceil(MCU rows of its longest segment / band) advances -- for a file of one thread segment
that is the file's MCU-row count divided by the band, rounded up."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import oracle_binding as ob
from conftest import golden
from lepton_amd import abi, corpus
from lepton_amd.codec import JpegImage, LepFile, LeptonError
from test_decode_rows_emulation import (FILL, check_failing_block, damaged_case, damaged_stream, fill_frame, frame_of, oracle_on_damaged,
                                        segment_mcu_rows, segment_rows)
from test_decode_rows_emulation import emu  # noqa: F401  (the module-scoped fixture that builds tests/emu/libcore_emu_decrows.so)

pytestmark = pytest.mark.gpu

CASES = {}


def case(name):
    """per fixture, once: a file-like object (desc, segments, the oracle's streams) and the oracle's frame decoded into a FILL-ed frame"""
    if name not in CASES:
        img = JpegImage(golden(name)[0])
        segs = img.plan()
        streams, _ = ob.oracle_encode(img.desc, segs)
        fill_frame(img.desc)
        ob.oracle_decode(img.desc, segs, streams)
        CASES[name] = (SimpleNamespace(desc=img.desc, segments=segs, streams=streams, image=img), frame_of(img.desc))
    return CASES[name]


def bands_of(f, s, band):
    n = segment_mcu_rows(f.desc, s)
    return 1 if band <= 0 else max(1, -(-n // band))


def decode_device(codec, files, fill=FILL):
    """lep_gpu_decode_device on device frames that start filled with `fill`; the frames are fetched into the files' host frames.
    Returns (return value, per-segment status)"""
    L, h = abi.lib(), codec.handle
    flat = [abi.Segment(i, s.luma_y_start, s.luma_y_end, s.is_last) for i, f in enumerate(files) for s in f.segments]
    streams = [st for f in files for st in f.streams]
    nseg = len(flat)
    blob, offs = b"", [0]
    for st in streams:
        blob += st + bytes(-len(st) % 256)
        offs.append(len(blob))
    owned = []

    def dmalloc(n):
        p = C.c_void_p()
        assert L.lep_gpu_malloc(h, n, C.byref(p)) == 0
        owned.append(p)
        return p

    try:
        dev = (abi.ImageDesc * len(files))(*[f.desc for f in files])
        for i, f in enumerate(files):
            for c in range(f.desc.ncomp):
                p = dmalloc(f.desc.nblocks(c) * 128 + 256)
                assert L.lep_gpu_memset(h, p, fill, f.desc.nblocks(c) * 128) == 0
                dev[i].blocks[c] = p.value
        d_streams, d_lens, d_status = dmalloc(len(blob) + 256), dmalloc(4 * nseg), dmalloc(4 * nseg)
        lens = (C.c_uint32 * nseg)(*[len(st) for st in streams])
        assert L.lep_gpu_memcpy_h2d(h, d_streams, blob, len(blob)) == 0 and L.lep_gpu_memcpy_h2d(h, d_lens, lens, 4 * nseg) == 0
        assert L.lep_gpu_memset(h, d_status, 0xff, 4 * nseg) == 0
        rc = L.lep_gpu_decode_device(h, dev, len(files), (abi.Segment * nseg)(*flat), nseg, d_streams, (C.c_uint64 * (nseg + 1))(*offs), d_lens, d_status, None)
        status = (C.c_int32 * nseg)()
        if rc == 0:
            assert L.lep_gpu_sync(h) == 0
            assert L.lep_gpu_memcpy_d2h(h, status, d_status, 4 * nseg) == 0
            for i, f in enumerate(files):
                for c in range(f.desc.ncomp):
                    assert L.lep_gpu_memcpy_d2h(h, f.desc.blocks[c], dev[i].blocks[c], f.desc.nblocks(c) * 128) == 0
        return rc, list(status)
    finally:
        for p in owned:
            L.lep_gpu_free(h, p)


def watch_session(codec, files, finals, band):
    """runs a session to its end, checking every segment after every advance; returns the per-segment lists of records"""
    segs = [(f, s) for f in files for s in f.segments]
    history = [[] for _ in segs]
    for f in files:
        fill_frame(f.desc)
    for progress in codec.decode_rows(files, band, fill=FILL):
        assert len(progress) == len(segs)
        now = {id(f): frame_of(f.desc) for f in files}
        for k, ((f, s), p) in enumerate(zip(segs, progress)):
            d, final = f.desc, finals[files.index(f)]
            if history[k]:
                before = history[k][-1]
                assert all(p.rows_done[c] >= before.rows_done[c] for c in range(d.ncomp))
                if before.status >= 0:   # finished (or failed) earlier: the record stays as it was
                    assert (p.status, list(p.rows_done), p.fail_component, p.fail_y, p.fail_x) == \
                           (before.status, list(before.rows_done), before.fail_component, before.fail_y, before.fail_x)
            history[k].append(p)
            for c in range(d.ncomp):
                first, last = segment_rows(d, s, c)
                lo = max(first, min(p.rows_done[c], last))
                assert np.array_equal(now[id(f)][c][first:lo], final[c][first:lo]), (k, c, "a row below rows_done is not final")
                if p.status <= 0:
                    assert (now[id(f)][c][lo:last] == FILL).all(), (k, c, "a row at or above rows_done is not untouched")
    return history


@pytest.mark.parametrize("band", [1, 3, 0])
@pytest.mark.parametrize("names", [("one_block_8x8", "c420_odd_203x149", "q30_256x256_4seg"), ("truncated", "gray_120x88")])
def test_session_equals_oracle_band_by_band(gpu_codec, names, band):
    files = [case(n)[0] for n in names]
    finals = [case(n)[1] for n in names]
    history = watch_session(gpu_codec, files, finals, band)
    assert b"lep_decode_v4_rows_kernel" in abi.lib().lep_gpu_last_kernel_name(gpu_codec.handle)
    segs = [(f, s) for f in files for s in f.segments]
    want_bands = [bands_of(f, s, band) for f, s in segs]
    assert all(len(h) == max(want_bands) for h in history)
    for h, n in zip(history, want_bands):   # every segment finishes at its own advance, clean
        assert [p.status for p in h] == [-1] * (n - 1) + [0] * (len(h) - n + 1)
        assert all(p.fail_component == p.fail_y == p.fail_x == -1 for p in h)
    if band == 1:
        assert len(set(want_bands)) > 1, "the launch is meant to hold segments that finish at different advances"
    for f, final in zip(files, finals):
        got = frame_of(f.desc)
        for c in range(f.desc.ncomp):
            assert np.array_equal(got[c], final[c])
    # the one-shot kernel on the same input: the same frames, every status zero
    for f in files:
        fill_frame(f.desc)
    rc, status = decode_device(gpu_codec, files)
    assert rc == 0 and not any(status)
    assert b"lep_decode_v4_kernel" in abi.lib().lep_gpu_last_kernel_name(gpu_codec.handle)
    for f, final in zip(files, finals):
        got = frame_of(f.desc)
        for c in range(f.desc.ncomp):
            assert np.array_equal(got[c], final[c])


def test_failing_block_on_the_gpu(gpu_codec):
    """seeds 0..9 of the 203 x 149 image's damaged streams at band 2, an intact c444_96x80 beside them in the same launch"""
    img, s, stream = damaged_case((203, 149))
    d = img.desc
    good, good_final = case("c444_96x80")
    refused = 0
    for seed in range(10):
        data = damaged_stream(stream, seed)
        oracle_rc, oracle_frame = oracle_on_damaged(d, s, data)
        refused += oracle_rc != 0
        bad = SimpleNamespace(desc=d, segments=[s], streams=[data])
        fill_frame(d)
        fill_frame(good.desc)
        last = None
        for progress in gpu_codec.decode_rows([bad, good], 2, fill=FILL):
            last = progress
        check_failing_block(d, s, oracle_rc, oracle_frame, last[0], frame_of(d))
        assert all(p.status == 0 and p.fail_component == -1 for p in last[1:])
        got = frame_of(good.desc)
        for c in range(good.desc.ncomp):
            assert np.array_equal(got[c], good_final[c])
    assert refused >= 8, refused   # so that the test cannot pass on nothing: the CPU test asks for 30 of 40, these are 10 of those 40


@pytest.mark.parametrize("waves", ["4", "8"])
def test_one_shot_decoder_on_damaged_streams(emu, monkeypatch, waves):
    """lep_decode_v4_kernel, both register-budget forms, on the same ten damaged streams, an intact c444_96x80 beside them in the launch:
    the status is the oracle's exit code, the frame (device frames start as FILL) is byte for byte the frame the same source leaves when
    it is stepped on the CPU (emu_decode_segment_v4) -- which is the oracle's frame except, at most, for the block the oracle stopped
    at -- and the neighbour is intact.  `verify` in lep_compress_batch rests on this answer."""
    from lepton_amd.codec import GpuCodec

    monkeypatch.setenv("LEP_DEC_WAVES", waves)
    img, s, stream = damaged_case((203, 149))
    d = img.desc
    good, good_final = case("c444_96x80")
    codec = GpuCodec(0)
    try:
        refused = 0
        for seed in range(10):
            data = damaged_stream(stream, seed)
            oracle_rc, oracle_frame = oracle_on_damaged(d, s, data)
            refused += oracle_rc != 0
            fill_frame(d)
            emu_rc = emu.emu_decode_segment_v4(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, data, len(data), None)
            emu_frame = frame_of(d)
            assert emu_rc == oracle_rc, seed
            differ = [(c,) + tuple(x) for c in range(d.ncomp) for x in np.argwhere((emu_frame[c] != oracle_frame[c]).any(axis=2))]
            assert len(differ) <= (1 if oracle_rc else 0), (seed, differ[:4])
            bad = SimpleNamespace(desc=d, segments=[s], streams=[data])
            fill_frame(d)
            fill_frame(good.desc)
            rc, status = decode_device(codec, [bad, good])
            assert rc == 0
            assert abi.lib().lep_gpu_last_kernel_name(codec.handle).decode() == "lep_decode_v4_kernel<%s>" % waves
            print("waves %s seed %d: oracle %d emulation %d gpu %s" % (waves, seed, oracle_rc, emu_rc, status))
            assert status == [oracle_rc] + [0] * len(good.segments), seed
            got = frame_of(d)
            for c in range(d.ncomp):
                assert np.array_equal(got[c], emu_frame[c]), (seed, c)
            got = frame_of(good.desc)
            for c in range(good.desc.ncomp):
                assert np.array_equal(got[c], good_final[c]), seed
        assert refused >= 8, refused   # so that the test cannot pass on nothing
    finally:
        codec.close()


def test_session_owns_its_workspace_set(gpu_codec):
    L, h = abi.lib(), gpu_codec.handle
    a, a_final = case("c420_odd_203x149")
    b, b_final = case("c444_96x80")

    def frames_equal(f, final):
        got = frame_of(f.desc)
        return all(np.array_equal(got[c], final[c]) for c in range(f.desc.ncomp))

    assert L.lep_gpu_use_arena(h, 0) == 0
    fill_frame(a.desc)
    session = gpu_codec.decode_rows([a], 1, fill=FILL)
    try:
        first = next(session)          # the session is open on set 0 and has made one advance
        assert first[0].status == -1
        rc, _ = decode_device(gpu_codec, [b])
        assert rc == abi_code("LEP_ASSERTION_FAILURE") and "decode session" in gpu_codec.last_error()
        assert L.lep_gpu_trim(h) == abi_code("LEP_ASSERTION_FAILURE") and "decode session" in gpu_codec.last_error()
        assert L.lep_gpu_use_arena(h, 1) == 0
        fill_frame(b.desc)
        rc, status = decode_device(gpu_codec, [b])      # the other set stays usable
        assert rc == 0 and not any(status) and frames_equal(b, b_final)
        assert L.lep_gpu_use_arena(h, 0) == 0
        with pytest.raises(LeptonError) as e:            # a second session on set 0
            next(gpu_codec.decode_rows([b], 1, fill=FILL))
        assert e.value.code == abi_code("LEP_ASSERTION_FAILURE")
        for _ in session:                                # the first one is none the worse for any of it
            pass
    finally:
        session.close()
        L.lep_gpu_use_arena(h, 0)
    assert frames_equal(a, a_final)
    # after the end everything on set 0 is accepted again, and a fresh session starts from cleared records and reset models
    assert L.lep_gpu_trim(h) == 0
    fill_frame(b.desc)
    rc, status = decode_device(gpu_codec, [b])
    assert rc == 0 and not any(status) and frames_equal(b, b_final)
    fill_frame(a.desc)
    history = watch_session(gpu_codec, [a], [a_final], 3)
    assert history[0][-1].status == 0 and frames_equal(a, a_final)


def abi_code(name):
    return {"LEP_ASSERTION_FAILURE": 1, "LEP_OS_ERROR": 33}[name]


def stream_case(lep, band, gpu_codec):
    f = LepFile(lep)
    want = gpu_codec.decompress(lep)
    chunks, stats = gpu_codec.decompress_stream(lep, band)
    assert b"".join(chunks) == want
    advances = max(bands_of(f, s, band) for s in f.segments)
    if len(f.segments) == 1:
        assert advances == -(-f.desc.mcu_rows // band)
    assert stats["advances"] == advances and advances > 1
    assert stats["advances_before_first_scan_byte"] == 1
    assert stats["bytes_before_last_advance"] > len(chunks[0])    # (the first sink call is the header)
    assert len(chunks) > 2


@pytest.mark.parametrize("band", [1, 4])
@pytest.mark.parametrize("name", ["c420_odd_203x149", "q30_256x256_4seg", "rst_c420_176x112"])
def test_decompress_stream_golden(gpu_codec, name, band):
    stream_case(golden(name)[1], band, gpu_codec)


def test_decompress_stream_1080p(gpu_codec):
    lep = gpu_codec.compress(corpus.synth_jpeg(1920, 1080, 10000))
    assert len(LepFile(lep).segments) == 8
    stream_case(lep, 8, gpu_codec)


def test_decompress_stream_of_a_progressive_file_is_one_chunk(gpu_codec):
    jpg, lep = golden("prog_c420_320x240")
    chunks, stats = gpu_codec.decompress_stream(lep, 4)
    assert chunks == [gpu_codec.decompress(lep)] and chunks[0] == jpg
    assert stats["advances"] == 0


def test_decompress_stream_sink_abort_closes_the_session(gpu_codec):
    L = abi.lib()
    jpg, lep = golden("q30_256x256_4seg")
    calls = []

    def sink(_user, data, n):
        calls.append(n)
        return 1 if len(calls) == 2 else 0

    stats = abi.StreamStats()
    rc = L.lep_decompress_stream(gpu_codec.handle, lep, len(lep), 1, abi.SINK_FN(sink), None, C.byref(stats))
    assert rc == abi_code("LEP_OS_ERROR") and len(calls) == 2
    assert gpu_codec.decompress(lep) == jpg            # the session was closed: set 0 takes launches again
    chunks, _ = gpu_codec.decompress_stream(lep, 1)
    assert b"".join(chunks) == jpg
