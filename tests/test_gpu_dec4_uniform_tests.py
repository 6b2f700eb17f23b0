"""The v4 decode kernels with their wave-uniform tests held as scalars and their lane-range tests written as selects (lep_dec4.h
LEP_DEC4_UNIFORM_TESTS / LEP_DEC4_LANE_SELECTS) on the GPU, in both register-budget builds (LEP_DEC_WAVES=4 / 8, a fresh codec handle each):
frames and per-segment statuses against the oracle, file by file and all in one launch, streams cut short, and the resumable kernel in
bands of one MCU row against the one-shot launch.  The lane-loop emulation cannot see an exec mask, so this is the test that catches a
select taken by the wrong lanes."""
import ctypes as C
from types import SimpleNamespace

import pytest

from lepton_amd import abi
from lepton_amd.codec import GpuCodec
from test_dec4_uniform_tests_emulation import IMAGES, case
from test_dec4_word_per_lane_emulation import (FILL, cut_case, cut_lengths, fill_frame, frame_of, oracle_on,
                                               same_frame_up_to_the_refused_block)
from test_gpu_decode_rows import decode_device

pytestmark = pytest.mark.gpu

NAMES = sorted(IMAGES)


@pytest.fixture(scope="module", params=["4", "8"])
def codec(request):
    mp = pytest.MonkeyPatch()
    mp.setenv("LEP_DEC_WAVES", request.param)
    c = GpuCodec(0)
    try:
        yield SimpleNamespace(codec=c, kernel="lep_decode_v4_kernel<%s>" % request.param)
    finally:
        c.close()
        mp.undo()


def file_of(name):
    img, segs, streams, _, frame = case(name)
    return SimpleNamespace(desc=img.desc, segments=segs, streams=streams, image=img), frame


def check_frames(files, frames):
    for f, frame in zip(files, frames):
        d = f.desc
        for c in range(d.ncomp):
            n = d.coded_blocks[c] * 128
            assert C.string_at(d.blocks[c], n) == frame[c][:n]


@pytest.mark.parametrize("names", [[n] for n in NAMES] + [NAMES], ids=lambda n: "+".join(n) if len(n) == 1 else "all_in_one_launch")
def test_frames_and_statuses_equal_the_oracle(codec, names):
    files, frames = zip(*[file_of(n) for n in names])
    for f in files:
        fill_frame(f.desc)
    rc, status = decode_device(codec.codec, list(files))
    assert rc == 0 and not any(status), (rc, status)
    assert codec.kernel in abi.lib().lep_gpu_last_kernel_name(codec.codec.handle).decode()
    check_frames(files, frames)


@pytest.mark.parametrize("k", [2, 8, 9])   # 2 bytes, 200 bytes, half the stream
def test_cut_streams_end_as_the_oracle_s_do(codec, k):
    img, s, stream = cut_case()
    d = img.desc
    data = stream[:cut_lengths(len(stream))[k]]
    want_rc, want_frame = oracle_on(d, s, data)
    fill_frame(d)
    rc, status = decode_device(codec.codec, [SimpleNamespace(desc=d, segments=[s], streams=[data])])
    assert rc == 0 and status == [want_rc]
    same_frame_up_to_the_refused_block(d, want_rc, frame_of(d), want_frame)


@pytest.mark.parametrize("name", ["c420_odd_203x149", "one_mcu_16x16_c420", "one_row_64x8_gray", "one_col_8x64_gray", "large_dc_64x48"])
def test_bands_of_one_mcu_row_equal_the_one_shot_launch(codec, name):
    f, frame = file_of(name)
    fill_frame(f.desc)
    rc, status = decode_device(codec.codec, [f])
    assert rc == 0 and not any(status)
    one_shot = frame_of(f.desc)
    fill_frame(f.desc)
    last = None
    for progress in codec.codec.decode_rows([f], 1, fill=FILL):
        last = progress
    assert last is not None and [p.status for p in last] == [0] * len(f.segments)
    assert b"lep_decode_v4_rows_kernel" in abi.lib().lep_gpu_last_kernel_name(codec.codec.handle)
    assert frame_of(f.desc) == one_shot
    check_frames([f], [frame])
