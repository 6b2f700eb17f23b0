"""The inputs of test_gpu_verify_refuses.py, checked without a GPU: every STREAM alteration named in verify_tamper_cases.py, made in the
oracle's own stream, must be one the oracle's decoder tells from the intact stream -- a non-zero exit code, or a frame that differs from the
input frame -- so that a `verify` that lets it through is wrong and not lucky; the offsets lie in the middle half of the stream, where the
suite's damaged streams (damaged_stream) have theirs; and the batches are cut as the GPU tests suppose."""
import ctypes as C

import numpy as np
import pytest

import oracle_binding as ob
import verify_tamper_cases as tc
from conftest import golden
from lepton_amd import abi
from lepton_amd.codec import JpegImage, LepFile
from test_decode_rows_emulation import frame_of, oracle_on_damaged


@pytest.mark.parametrize("name,offset,mask,oracle_rc", tc.STREAM_CASES)
def test_oracle_tells_the_altered_stream_from_the_intact_one(name, offset, mask, oracle_rc):
    jpg, lep = golden(name)
    img = JpegImage(jpg)
    segs = img.plan()
    frame = frame_of(img.desc)
    streams, _ = ob.oracle_encode(img.desc, segs)
    assert len(streams) == 1 and streams == LepFile(lep).streams      # the stream the GPU writes, byte for byte
    stream = streams[0]
    assert len(stream) // 4 <= offset < 3 * len(stream) // 4 and 0 < mask < 256
    rc, intact = oracle_on_damaged(img.desc, segs[0], stream)
    assert rc == 0 and all(np.array_equal(intact[c], frame[c]) for c in range(img.desc.ncomp))
    bad = bytearray(stream)
    bad[offset] ^= mask
    rc, got = oracle_on_damaged(img.desc, segs[0], bytes(bad))
    assert rc == oracle_rc
    assert rc != 0 or any(not np.array_equal(got[c], frame[c]) for c in range(img.desc.ncomp))


def test_cases_cover_both_signals():
    """one alteration at least that ends the decode with a status, and one that only the frame comparison can see"""
    assert {rc != 0 for _, _, _, rc in tc.STREAM_CASES} == {True, False}
    assert {"c420_160x120", "gray_120x88", "prog_c420_320x240"} <= {n for n, _, _, _ in tc.STREAM_CASES}


@pytest.mark.parametrize("target", sorted({n for n, _, _, _ in tc.STREAM_CASES} | {n for n, _ in tc.SCRATCH_CASES}))
def test_batches_are_cut_into_three_chunks_with_the_target_in_the_second(target):
    L = abi.lib()
    names = tc.batch_names(target)
    assert len(names) == 12 and names[tc.TARGET] == target and names.count(target) == 1
    jpgs = [golden(n)[0] for n in names]
    n = len(jpgs)
    file_bytes = (C.c_size_t * n)(*[len(j) for j in jpgs])
    frame_bytes = (C.c_size_t * n)()
    for i, j in enumerate(jpgs):
        fb = C.c_size_t()
        assert L.lep_jpeg_peek_frame_bytes(j, len(j), C.byref(fb)) == 0
        frame_bytes[i] = fb.value
    opt = abi.BatchOptions(0, 1, 0, 0, tc.CHUNK_IMAGES)
    first = (C.c_int * (n + 2))()
    k = L.lep_batch_plan(file_bytes, frame_bytes, n, C.byref(opt), first, n + 2)
    assert k == 3 and list(first[:4]) == [0, 4, 8, 12]
    assert first[1] <= tc.TARGET < first[2]
