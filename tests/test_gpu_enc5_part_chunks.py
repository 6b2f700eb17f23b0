"""The stitched writer with its chunks cut at the boundaries of gather's parts, a part's chunks ranged / linked / coded beside the
gather of the next (lep_gpu.hip launch_enc5, LEP_ENC5_WSCHED=beside; lep_enc5.h part_chunk_cut) on the MI355X: the frames of
tests/enc5_gather_frames.py at 64 / 65 / 129 blocks per row -- segments of one, two and a few tiles, fewer tiles than parts -- and one
frame whose parts are longer than the warm-up of 16,384 bins, through lep_gpu_encode_host in launches of 8 and of 72 segments, at 8
parts of 1 and of 4 chunks and at 3 parts: streams and lengths are the oracle's, the device decoder returns the frames, and a segment
the coder refuses keeps its exit code."""
import ctypes as C
import os

import pytest

import oracle_binding as ob
from enc5_gather_frames import CONTENTS, frame
from lepton_amd.codec import GpuCodec, LepFile, LeptonError

SHAPES = [(64, 4, False), (65, 2, False), (129, 4, False), (65, 3, True)]
LARGE = (129, 16, False, "alternating")   # ~1,000 bins per dense block, every other block: a part of a segment is far beyond 16,384 bins
CASES = {}
KNOBS = ("LEP_ENC5_MIN", "LEP_ENC5_WMAXSEG", "LEP_ENC5_WSCHED", "LEP_ENC5_PARTS", "LEP_ENC5_WPARTCHUNKS")


def cases():
    """once: [(image, plan, oracle streams, frame bytes)] of every shape x content, the large frame last"""
    if not CASES:
        out = []
        for args in [shape + (content,) for shape in SHAPES for content in CONTENTS] + [LARGE]:
            img = frame(*args)
            plan = img.plan()
            want, _ = ob.oracle_encode(img.desc, plan)
            d = img.desc
            out.append((img, plan, want, [C.string_at(d.blocks[c], d.coded_blocks[c] * 128) for c in range(d.ncomp)]))
        CASES["all"] = out
    return CASES["all"]


@pytest.fixture(scope="module", params=[(8, 1), (8, 4), (3, 4), (2, 32)], ids=["8_parts_1_chunk", "8_parts_4_chunks", "3_parts_4_chunks", "2_parts_32_chunks"])
def codec(request):
    old = {k: os.environ.get(k) for k in KNOBS}
    os.environ.update({"LEP_ENC5_MIN": "1", "LEP_ENC5_WMAXSEG": "0", "LEP_ENC5_WSCHED": "beside", "LEP_ENC5_PARTS": str(request.param[0]),
                       "LEP_ENC5_WPARTCHUNKS": str(request.param[1])})
    try:
        return GpuCodec(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def launch_of(nseg):
    """the large frame and as many of the sixteen one-segment frames, in turn, as make nseg segments"""
    base = cases()
    small, large = base[:-1], base[-1]
    assert all(len(p) == 1 for _, p, _, _ in small) and len(small) == 16 and len(large[1]) < 8
    group = [large] + (small * 5)[:nseg - len(large[1])]
    assert sum(len(g[1]) for g in group) == nseg
    return group


@pytest.mark.gpu
@pytest.mark.parametrize("nseg", [8, 72])
def test_gpu_part_chunk_streams_equal_the_oracle_and_round_trip(codec, nseg):
    small = cases()[:-1]
    groups = [launch_of(nseg)] + ([small[:8], small[8:]] if nseg == 8 else [])   # (at 8 segments: every small frame too)
    for group in groups:
        got = codec.encode([g[0] for g in group], [g[1] for g in group])
        assert b"part chunks beside gather" in codec._L.lep_gpu_last_kernel_name(codec.handle)
        for (img, plan, want, fr), streams in zip(group, got):
            assert [len(s) for s in streams] == [len(w) for w in want]
            assert streams == want
    # round trip: the device decoder returns the frames the streams were made from
    files = [LepFile(img.write_lep(want)) for img, _, want, _ in cases()]
    codec.decode(files)
    for f, (_, _, _, fr) in zip(files, cases()):
        for c in range(f.desc.ncomp):
            assert C.string_at(f.desc.blocks[c], len(fr[c])) == fr[c]


@pytest.mark.gpu
def test_gpu_part_chunks_keep_a_refused_segment_s_exit_code(codec):
    """a coefficient the coder does not take (exit code 6, set by the emit walk) among segments it does: the code comes through the
    chunk phases, which skip the segment, and the stitch"""
    group = launch_of(8)
    bad = frame(65, 2, False, "one_per_block")
    C.cast(bad.desc.blocks[0], C.POINTER(C.c_int16))[64 * 3 + 5] = 4096
    with pytest.raises(RuntimeError, match="exit code 6"):
        ob.oracle_encode(bad.desc, bad.plan())
    with pytest.raises(LeptonError) as e:
        codec.encode([g[0] for g in group[:5]] + [bad] + [g[0] for g in group[5:]], [g[1] for g in group[:5]] + [bad.plan()] + [g[1] for g in group[5:]])
    assert e.value.code == 6
    assert b"part chunks beside gather" in codec._L.lep_gpu_last_kernel_name(codec.handle)
