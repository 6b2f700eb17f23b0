"""The gather kernel's staging ring and its drains at check points (lep_enc5.h Walk5::put_bin / drain / flush_bin) on the MI355X: the frames of
tests/enc5_gather_frames.py at 64 / 65 / 129 blocks per row through lep_gpu_encode_device, in launches of 8 and of 72 segments, with the
lane-per-segment writer beside gather (LEP_ENC5_WCHUNKS=0) and with the stitched writer: streams and lengths are the oracle's, and
lep_gpu_decode_device returns the frames."""
import ctypes as C
import os

import pytest

import oracle_binding as ob
from enc5_gather_frames import CONTENTS, frame
from lepton_amd.codec import GpuCodec, LepFile

SHAPES = [(64, 4, False), (65, 2, False), (129, 4, False), (65, 3, True)]
CASES = {}


def cases():
    """once: [(image, plan, oracle streams, frame bytes)] of every shape x content"""
    if not CASES:
        out = []
        for shape in SHAPES:
            for content in CONTENTS:
                img = frame(*shape, content)
                plan = img.plan()
                want, _ = ob.oracle_encode(img.desc, plan)
                d = img.desc
                out.append((img, plan, want, [C.string_at(d.blocks[c], d.coded_blocks[c] * 128) for c in range(d.ncomp)]))
        CASES["all"] = out
    return CASES["all"]


@pytest.fixture(scope="module", params=["0", "64"], ids=["lane_per_segment_writer", "stitched_writer"])
def codec(request):
    old = {k: os.environ.get(k) for k in ("LEP_ENC5_MIN", "LEP_ENC5_WCHUNKS")}
    os.environ["LEP_ENC5_MIN"] = "1"
    os.environ["LEP_ENC5_WCHUNKS"] = request.param
    try:
        return GpuCodec(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.mark.gpu
@pytest.mark.parametrize("nseg", [8, 72])
def test_gpu_gather_streams_equal_the_oracle_and_round_trip(codec, nseg):
    """launches of nseg segments (one per frame; the 72 are the sixteen frames four and a half times)"""
    base = cases()
    assert all(len(p) == 1 for _, p, _, _ in base) and len(base) == 16   # (frames this small are one segment each)
    groups = [base[:8], base[8:]] if nseg == 8 else [(base * 5)[:72]]
    for group in groups:
        assert len(group) == nseg
        got = codec.encode([g[0] for g in group], [g[1] for g in group])
        assert b"enc5" in codec._L.lep_gpu_last_kernel_name(codec.handle)
        for (img, plan, want, fr), streams in zip(group, got):
            assert [len(s) for s in streams] == [len(w) for w in want]
            assert streams == want
    # round trip: the device decoder returns the frames the streams were made from
    files = [LepFile(img.write_lep(want)) for img, _, want, _ in base]
    codec.decode(files)
    for f, (_, _, _, fr) in zip(files, base):
        for c in range(f.desc.ncomp):
            assert C.string_at(f.desc.blocks[c], len(fr[c])) == fr[c]
