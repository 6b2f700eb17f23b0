"""lep_gpu_samples_device (lepton_amd/csrc/lep_samples.h) on the GPU, through GpuCodec.samples: the in-domain frames of
tests/samples_frames.py -- the domain's corners included -- as images of one, two and three components, several images of different
geometry in one launch, at both scales, pitches equal to the width and wider, whole planes and row ranges.  Every sample must equal
tests/samples_ref.py; the canary bytes in front of and behind each plane, the pitch padding and the rows outside a range must be
untouched; every refusal returns its code with an error text and writes nothing."""
import ctypes as C

import numpy as np
import pytest

import samples_frames as sf
from lepton_amd import abi
from lepton_amd.codec import GpuCodec, LeptonError

pytestmark = pytest.mark.gpu

M = GpuCodec.SAMPLES_MARGIN
assert GpuCodec.SAMPLES_CANARY == sf.CANARY


def desc_of(comps):
    """comps: [(q, blocks)] -> an ImageDesc with host pointers into the arrays (which the caller keeps alive)"""
    d = abi.ImageDesc()
    d.ncomp = len(comps)
    d.mcu_rows = comps[0][1].shape[0]
    for c, (q, blocks) in enumerate(comps):
        assert blocks.dtype == np.int16 and blocks.flags["C_CONTIGUOUS"]
        d.width_blocks[c], d.height_blocks[c] = blocks.shape[1], blocks.shape[0]
        d.coded_blocks[c], d.coded_height[c] = blocks.shape[0] * blocks.shape[1], blocks.shape[0]
        for z in range(64):
            d.qtable_zigzag[c][z] = int(q[z])
        d.blocks[c] = blocks.ctypes.data
    return d


@pytest.fixture(scope="module")
def frames():
    return {n: (q, np.ascontiguousarray(b)) for n, q, b in sf.in_domain()}


@pytest.fixture(scope="module")
def three_images(frames):
    """different geometry: three components with a chroma grid half the luma's; one component, one block wide; the corners beside two others"""
    y = sf.random_frame(18, 4, 1)
    cb, cr = sf.random_frame(9, 2, 2), sf.random_frame(9, 2, 3)
    return [[y, cb, cr], [frames["random_1x3"]], [frames["corners"], frames["random_8x3"], frames["random_17x1"]]]


def check(bufs, images, scale, rows=None, pitch=None):
    for i, comps in enumerate(images):
        assert len(bufs[i]) == len(comps)
        for c, (q, blocks) in enumerate(comps):
            h, w = sf.plane_size(blocks, scale)
            p = pitch[i][c] if pitch is not None else w
            r = rows[i][c] if rows is not None else (0, blocks.shape[0])
            buf = np.frombuffer(bufs[i][c], dtype=np.uint8)
            assert len(buf) == M + h * p + M
            assert (buf[:M] == sf.CANARY).all(), "bytes in front of plane (%d, %d) were written" % (i, c)
            assert (buf[M + h * p:] == sf.CANARY).all(), "bytes behind plane (%d, %d) were written" % (i, c)
            got, want = buf[M:M + h * p].reshape(h, p), sf.expected_rows(q, blocks, scale, r, p)
            assert np.array_equal(got, want), (i, c, scale, r, p, int((got != want).sum()))


def run(codec, images, scale, rows=None, pitch=None):
    return codec.samples([desc_of(comps) for comps in images], scale, rows, pitch)


@pytest.mark.parametrize("scale", [1, 8])
def test_every_in_domain_frame_equals_the_definition(gpu_codec, frames, scale):
    images = [[f] for f in frames.values()]
    check(run(gpu_codec, images, scale), images, scale)


@pytest.mark.parametrize("scale", [1, 8])
@pytest.mark.parametrize("extra", [0, 24, 3])
def test_three_images_of_different_geometry_in_one_launch(gpu_codec, three_images, scale, extra):
    """pitch = the width, 24 bytes more, and 3 bytes more (planes and rows that are not 8-byte aligned: the byte stores)"""
    pitch = [[sf.plane_size(b, scale)[1] + extra for _, b in comps] for comps in three_images]
    check(run(gpu_codec, three_images, scale, pitch=pitch), three_images, scale, pitch=pitch)


@pytest.mark.parametrize("scale", [1, 8])
def test_row_ranges(gpu_codec, three_images, scale):
    def ranges(pick):
        return [[pick(b.shape[0]) for _, b in comps] for comps in three_images]

    pitch = [[sf.plane_size(b, scale)[1] + 24 for _, b in comps] for comps in three_images]
    middle = ranges(lambda h: (1, h - 1) if h >= 3 else (0, h))
    check(run(gpu_codec, three_images, scale, rows=middle, pitch=pitch), three_images, scale, rows=middle, pitch=pitch)
    empty = ranges(lambda h: (h // 2, h // 2))
    check(run(gpu_codec, three_images, scale, rows=empty, pitch=pitch), three_images, scale, rows=empty, pitch=pitch)
    # two consecutive ranges: each writes its rows and nothing else, together they are the whole plane
    front, back = ranges(lambda h: (0, (h + 1) // 2)), ranges(lambda h: ((h + 1) // 2, h))
    a, b = run(gpu_codec, three_images, scale, rows=front, pitch=pitch), run(gpu_codec, three_images, scale, rows=back, pitch=pitch)
    check(a, three_images, scale, rows=front, pitch=pitch)
    check(b, three_images, scale, rows=back, pitch=pitch)
    for i, comps in enumerate(three_images):
        for c, (q, blocks) in enumerate(comps):
            ba, bb = np.frombuffer(a[i][c], dtype=np.uint8), np.frombuffer(b[i][c], dtype=np.uint8)
            cut = M + front[i][c][1] * (8 // scale) * pitch[i][c]
            whole = np.concatenate([ba[:cut], bb[cut:]])
            want = np.concatenate([np.full(M, sf.CANARY, np.uint8), sf.expected_rows(q, blocks, scale, (0, blocks.shape[0]), pitch[i][c]).reshape(-1), np.full(M, sf.CANARY, np.uint8)])
            assert np.array_equal(whole, want)


def refused(codec, images, scale, rows=None, pitch=None):
    with pytest.raises(LeptonError) as e:
        run(codec, images, scale, rows, pitch)
    assert e.value.code == 1, e.value                       # LEP_ASSERTION_FAILURE
    assert "lep_gpu_samples_device" in str(e.value) and codec.last_error().startswith("lep_gpu_samples_device: ")
    for per_image in e.value.buffers:
        for buf in per_image:
            assert (np.frombuffer(buf, dtype=np.uint8) == sf.CANARY).all(), "a refused call wrote into a plane"
    return codec.last_error()


def test_refusals_write_nothing(gpu_codec, three_images):
    assert "scale" in refused(gpu_codec, three_images, 2)
    assert "scale" in refused(gpu_codec, three_images, 0)
    for scale in (1, 8):
        width = [[sf.plane_size(b, scale)[1] for _, b in comps] for comps in three_images]
        short = [list(p) for p in width]
        short[2][1] -= 1
        assert "pitch" in refused(gpu_codec, three_images, scale, pitch=short)
        whole = [[(0, b.shape[0]) for _, b in comps] for comps in three_images]
        for bad in ((0, three_images[0][1][1].shape[0] + 1), (-1, 1), (2, 1)):
            rows = [list(r) for r in whole]
            rows[0][1] = bad
            assert "rows" in refused(gpu_codec, three_images, scale, rows=rows)
