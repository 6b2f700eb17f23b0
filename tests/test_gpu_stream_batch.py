"""lep_decompress_batch_stream on the GPU: many files in one decode session, every band's completed rows written by the lane scan writer on
the device, the band's bytes packed and fetched -- held against the golden JPEGs, against lep_decompress's exit codes, and against
lep_decompress_stream's choice of which files are streamed; then the same through the serving daemon."""
import contextlib
import ctypes as C
import os
import uuid

import pytest

from conftest import golden
from lepton_amd import abi, corpus
from lepton_amd.codec import GpuCodec, LeptonError, LepFile

pytestmark = pytest.mark.gpu

NAMES = ["c420_odd_203x149", "q30_256x256_4seg", "rst_c420_176x112", "one_block_8x8", "gray_120x88", "truncated", "prog_c420_320x240"]
LEP_OS_ERROR = 33


@contextlib.contextmanager
def environment(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def streamed_alone(gpu_codec):
    """per golden file, once: does lep_decompress_stream decode it in a session?"""
    return {name: gpu_codec.decompress_stream(golden(name)[1], 4)[1]["advances"] > 0 for name in NAMES}


def front_rows(lep):
    """MCU rows of the file's first thread segment"""
    f = LepFile(lep)
    img, segs = abi.HuffImage(), (abi.HuffSegment * abi.MAX_SEGMENTS)()
    nseg, ok = C.c_int(0), C.c_int(0)
    assert abi.lib().lep_file_recode_plan(f.handle, C.byref(img), segs, C.byref(nseg), C.byref(ok)) == 0 and ok.value
    return segs[0].mcu_row1 - segs[0].mcu_row0


@pytest.mark.parametrize("pack", [None, "0"])
@pytest.mark.parametrize("band", [1, 4, 0])
def test_batch_of_golden_files(streamed_alone, band, pack):
    with environment(LEP_STREAM_PACK=pack):
        codec = GpuCodec(0)   # (the switch is read when the codec is made)
    try:
        assert abi.lib().lep_gpu_stream_pack(codec.handle) == (0 if pack == "0" else 1)
        leps = [golden(name)[1] for name in NAMES]
        pieces, status, stats = codec.decompress_batch_stream(leps, band)
        assert status == [0] * len(NAMES)
        for name, p in zip(NAMES, pieces):
            assert b"".join(p) == golden(name)[0], name
        streamed = [name for name in NAMES if streamed_alone[name]]
        assert stats["files_streamed"] == len(streamed) and stats["files_whole"] == len(NAMES) - len(streamed)
        assert len(streamed) >= 3
        for name, p in zip(NAMES, pieces):
            if name not in streamed:
                assert len(p) == 1, name
        assert stats["sessions"] == 1 and stats["frame_bytes_down"] == 0
        assert stats["writer_launches"] >= 1 and stats["writer_launches"] <= stats["advances"]
        assert stats["scan_bytes_down"] > 0
        if band == 1:
            assert len(pieces[NAMES.index("q30_256x256_4seg")]) > 2
        want = sum(1 for name in streamed if band > 0 and front_rows(golden(name)[1]) > band)
        assert stats["files_first_scan_byte_before_last_advance"] == want
    finally:
        codec.close()


def test_two_sessions(gpu_codec):
    jpg = corpus.synth_jpeg(1920, 1080, 10000)
    lep = gpu_codec.compress(jpg)
    assert len(LepFile(lep).segments) == 8
    with environment(LEP_STREAM_SESSION_FILES="1"):
        pieces, status, stats = gpu_codec.decompress_batch_stream([lep, lep], 8)
    assert status == [0, 0] and stats["sessions"] == 2 and stats["files_streamed"] == 2
    assert b"".join(pieces[0]) == jpg and b"".join(pieces[1]) == jpg
    assert len(pieces[0]) > 2 and stats["frame_bytes_down"] == 0


def damaged_lep(gpu_codec):
    """a one-segment file whose stream is damaged as test_failing_block_on_the_gpu damages its own: (.lep, lep_decompress's exit code)"""
    from test_decode_rows_emulation import damaged_case, damaged_stream

    img, _seg, stream = damaged_case((203, 149))
    for seed in range(10):
        lep = img.write_lep([damaged_stream(stream, seed)])
        try:
            gpu_codec.decompress(lep)
        except LeptonError as e:
            return lep, e.code
    raise AssertionError("no damaged stream was refused")


def test_damaged_stream_between_two_good_files(gpu_codec):
    bad, code = damaged_lep(gpu_codec)
    assert code != 0
    (jpg_a, lep_a), (jpg_b, lep_b) = golden("q30_256x256_4seg"), golden("c420_odd_203x149")
    pieces, status, stats = gpu_codec.decompress_batch_stream([lep_a, bad, lep_b], 2)
    assert status == [0, code, 0]
    assert stats["files_streamed"] == 3
    assert b"".join(pieces[0]) == jpg_a and b"".join(pieces[2]) == jpg_b
    pieces, status, _ = gpu_codec.decompress_batch_stream([lep_b, lep_a], 2)    # the session was closed
    assert status == [0, 0] and b"".join(pieces[0]) == jpg_b and b"".join(pieces[1]) == jpg_a


def test_sink_abort_fails_that_file_only(gpu_codec):
    L = abi.lib()
    names = ["c420_odd_203x149", "q30_256x256_4seg", "rst_c420_176x112"]
    leps = [golden(n)[1] for n in names]
    ins = (abi.Bytes * 3)()
    keep = [C.create_string_buffer(b, len(b)) for b in leps]
    for i, b in enumerate(keep):
        ins[i].data, ins[i].len, ins[i].cap = C.cast(b, C.c_void_p).value, len(leps[i]), len(leps[i])
    pieces = [[], [], []]

    def sink(_user, i, data, n):
        pieces[i].append(C.string_at(data, n))
        return 1 if i == 1 else 0

    status = (C.c_int32 * 3)()
    stats = abi.BatchStreamStats()
    opt = abi.BatchOptions()
    rc = L.lep_decompress_batch_stream(gpu_codec.handle, ins, 3, 1, abi.BATCH_SINK_FN(sink), None, status, C.byref(opt), C.byref(stats))
    assert rc == 0 and list(status) == [0, LEP_OS_ERROR, 0]
    assert len(pieces[1]) == 1, "nothing is sunk for a file after its sink said that the receiver is gone"
    assert b"".join(pieces[0]) == golden(names[0])[0] and b"".join(pieces[2]) == golden(names[2])[0]
    # a decode launch on the same arena set is not refused: the session was closed
    f = LepFile(leps[0])
    gpu_codec.decode([f])
    assert gpu_codec.decompress(leps[1]) == golden(names[1])[0]


def test_server_streams_a_file(gpu_codec):
    from lepton_amd.serve import Server, request, zlib0_wrap

    jpg, lep = golden("q30_256x256_4seg")
    path = "/tmp/lep-%s" % uuid.uuid4().hex[:12]
    with Server(path, gpu=gpu_codec, stream_band_mcu_rows=1) as srv:
        assert request(path, lep) == jpg
        st = srv.stats()
        assert st["streamed"] == 1 and st["answered"] == 1 and st["failed"] == 0
        assert request(path, jpg) == lep                       # a compress request: today's path
        assert request(path + ".z0", lep) == zlib0_wrap(jpg)   # a zlib answer: today's path
        st = srv.stats()
        assert st["streamed"] == 1 and st["answered"] == 3
