"""Streamed decompress on the GPU over the layouts it takes besides whole interleaved files: one-component files (plain, with a restart interval
per row, with sampling factors and padding blocks, of several thread segments), -startbyte / -trunc slices ('Y') and files cut inside their
scan ('Z' and 'Y', one segment and four).  Every one of them is decoded in a session, written band by band by the lane scan writer and
finished without a frame crossing PCIe; the bytes are lep_decompress's.  Then the single-file call, a batch mixed with files that are not
streamed, and the serving daemon."""
import ctypes as C
import uuid

import pytest

from conftest import golden
from lepton_amd import abi
from lepton_amd.codec import LepFile
from stream_layout_cases import FIXTURES, GENERATED, generated_gray, lep_of

pytestmark = pytest.mark.gpu

NAMES = list(FIXTURES) + [GENERATED]


@pytest.fixture(scope="module")
def want(gpu_codec):
    """per file, once: what lep_decompress restores -- the golden JPEG, or the part of it a slice was made from"""
    out = {}
    for name in NAMES + ["prog_c420_320x240", "c420_odd_203x149"]:
        out[name] = gpu_codec.decompress(lep_of(name))
        jpg = generated_gray()[0] if name == GENERATED else golden(name)[0]
        assert (out[name] in jpg and len(out[name]) > 0) if "slice" in FIXTURES.get(name, "") else (out[name] == jpg), name
    return out


def front_mcu_rows(lep):
    """MCU rows of the file's first thread segment, as test_gpu_stream_batch.py::front_rows counts them -- and for a one-component file,
    whose planned rows are block rows while a band is counted in MCU rows, those block rows over the frame's block rows per MCU row"""
    f = LepFile(lep)
    img, segs = abi.HuffImage(), (abi.HuffSegment * abi.MAX_SEGMENTS)()
    nseg, ok = C.c_int(0), C.c_int(0)
    assert abi.lib().lep_file_recode_plan(f.handle, C.byref(img), segs, C.byref(nseg), C.byref(ok)) == 0 and ok.value
    unit = max(f.desc.height_blocks[0] // f.desc.mcu_rows, 1) if img.ncomp == 1 else 1
    return -(-segs[0].mcu_row1 // unit) - segs[0].mcu_row0 // unit


@pytest.mark.parametrize("band", [1, 4, 0])
def test_batch_of_the_layouts(gpu_codec, want, band):
    leps = [lep_of(name) for name in NAMES]
    pieces, status, stats = gpu_codec.decompress_batch_stream(leps, band)
    print(band, status, stats, [len(p) for p in pieces])
    assert status == [0] * len(NAMES)
    for name, p in zip(NAMES, pieces):
        assert b"".join(p) == want[name], name
    assert stats["files_streamed"] == len(NAMES) and stats["files_whole"] == 0
    assert stats["sessions"] == 1
    assert stats["frame_bytes_down"] == 0
    first_early = sum(1 for lep in leps if band > 0 and front_mcu_rows(lep) > band)
    assert stats["files_first_scan_byte_before_last_advance"] == first_early
    if band == 1:
        assert first_early >= 8 and len(pieces[NAMES.index("lay_gray22_80x56")]) > 3


@pytest.mark.parametrize("name", NAMES)
def test_single_file(gpu_codec, want, name):
    chunks, stats = gpu_codec.decompress_stream(lep_of(name), 2)
    print(name, stats, len(chunks))
    assert stats["advances"] > 0
    assert b"".join(chunks) == want[name]


def test_mixed_batch(gpu_codec, want):
    names = list(FIXTURES) + ["prog_c420_320x240", "c420_odd_203x149"]
    pieces, status, stats = gpu_codec.decompress_batch_stream([lep_of(name) for name in names], 2)
    print(status, stats)
    assert status == [0] * len(names)
    for name, p in zip(names, pieces):
        assert b"".join(p) == want[name], name
    assert len(pieces[names.index("prog_c420_320x240")]) == 1
    assert stats["files_whole"] == 1 and stats["files_streamed"] == len(names) - 1 and stats["frame_bytes_down"] == 0


def test_server_streams_a_cut_slice(gpu_codec, want):
    from lepton_amd.serve import Server, request

    path = "/tmp/lep-%s" % uuid.uuid4().hex[:12]
    with Server(path, gpu=gpu_codec, stream_band_mcu_rows=1) as srv:
        before = srv.stats()["streamed"]
        assert request(path, lep_of("slice_4seg_q97")) == want["slice_4seg_q97"]
        st = srv.stats()
        assert st["streamed"] == before + 1 and st["failed"] == 0
