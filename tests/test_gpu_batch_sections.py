"""Both batch pipelines on the MI355X with EVERY section of the compressor's scan arena non-empty in the same chunk (sequential scans, a
restart table behind one, progressive scans, a restart table behind one of those, and under `verify` both kinds of reference copies;
lep_batch_layout.h lay_out_scan_arena), beside a file that only the host parser takes and one that is no JPEG: the smallest shape at
which a slip in the layout can show.  A layout mistake can hide behind a fallback that still returns the right bytes, so the fallback
counters are held too.  The list of files was checked against the commit before the pipelines were cut into stages: there, too, none
of them takes a second chance or the per-file path, and the same five are coded by the GPU Huffman kernels in both directions."""
import numpy as np
import pytest

import jpeg_writer as jw
from conftest import golden
from lepton_amd import corpus
from lepton_amd.codec import LeptonError

pytestmark = pytest.mark.gpu

C420 = [(1, 2, 2, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)]


def _files():
    """(name, bytes, coded by the GPU Huffman kernels)"""
    return [
        ("baseline 4:2:0", corpus.synth_jpeg(320, 240, 501), True),
        ("baseline with a restart interval", jw.write_baseline(333, 250, C420, np.random.default_rng(5), density=0.1, restart_interval=21)[0], True),
        ("grey", golden("gray_120x88")[0], True),
        ("progressive", corpus.synth_jpeg(256, 256, 42, progressive=True), True),
        ("progressive with restart intervals", golden("prog_c422_rst_176x112")[0], True),
        ("host parser only", golden("prog_truncated_mid")[0], False),
        ("no JPEG", b"not a jpeg at all", False),
    ]


FILES = _files()
JPGS = [f[1] for f in FILES]
ON_GPU = sum(1 for f in FILES if f[2])


@pytest.fixture(scope="module")
def per_file(gpu_codec):
    """the per-file calls, once: (status, .lep bytes or None)"""
    out = []
    for jpg in JPGS:
        try:
            out.append((0, gpu_codec.compress(jpg)))
        except LeptonError as e:
            out.append((e.code, None))
    assert [st == 0 for st, _ in out] == [True] * 6 + [False]
    return out


@pytest.mark.parametrize("verify", [False, True], ids=["plain", "verify"])
@pytest.mark.parametrize("chunk_images", [0, 2], ids=["one_chunk", "three_chunks"])
def test_every_section_of_the_scan_arena_in_one_chunk(gpu_codec, per_file, chunk_images, verify):
    # chunk_images 2: the chunking counts the files with a frame, so the six JPEGs make three chunks of two in both directions (the file
    # that is no JPEG rides with the last): the third chunk takes slot 0 again, behind a chunk on slot 1
    before = gpu_codec.scan_second_chances()
    leps, status, stats = gpu_codec.compress_batch(JPGS, verify=verify, chunk_images=chunk_images)
    print("compress", chunk_images, verify, status, {k: stats[k] for k in ("gpu_huffman_files", "redone_files", "gpu_verified_scans")}, gpu_codec.scan_second_chances() - before)
    assert status == [st for st, _ in per_file]
    assert leps == [lep for _, lep in per_file]
    assert stats["redone_files"] == 0
    assert gpu_codec.scan_second_chances() == before
    assert stats["gpu_huffman_files"] == ON_GPU
    if verify:
        assert stats["gpu_verified_scans"] > 0
    good = [lep for lep in leps if lep is not None]
    back, status2, stats2 = gpu_codec.decompress_batch(good, chunk_images=chunk_images)
    print("decompress", chunk_images, status2, stats2["gpu_huffman_files"])
    assert status2 == [0] * len(good)
    assert back == [jpg for jpg, (st, _) in zip(JPGS, per_file) if st == 0]
    assert stats2["gpu_huffman_files"] == ON_GPU
