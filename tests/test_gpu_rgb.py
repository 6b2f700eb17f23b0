"""lep_gpu_rgb_device (lepton_amd/csrc/lep_rgb.h) on the GPU, through GpuCodec.rgb: the images of tests/rgb_cases.py -- the ones the
emulation steps on the CPU: every layout, widths 1..8 and round a unit's 256 pixels, heights 1, 2, 3 and 17, pitches that equal the row,
run wider on dwords and run wider by an odd count, row ranges, several images of different geometry in one launch -- on random planes
with 0 and 255 among them.  Every pixel must equal tests/rgb_ref.py; the canary bytes in front of and behind each output, the pitch
padding and the rows outside a range must be untouched.  Every refusal returns its code with a text and writes nothing."""
import copy

import numpy as np
import pytest

import rgb_cases
from lepton_amd.codec import GpuCodec, LeptonError

pytestmark = pytest.mark.gpu

M = GpuCodec.SAMPLES_MARGIN
assert GpuCodec.SAMPLES_CANARY == rgb_cases.CANARY


@pytest.fixture(scope="module")
def tables():
    return rgb_cases.tables()


def check(bufs, images, name=""):
    assert len(bufs) == len(images)
    for i, (buf, m) in enumerate(zip(bufs, images)):
        got = np.frombuffer(buf, dtype=np.uint8)
        n = m["rgb_pitch"] * m["height"]
        assert len(got) == n + 2 * M
        assert (got[:M] == rgb_cases.CANARY).all() and (got[M + n:] == rgb_cases.CANARY).all(), (name, i, "a margin was written")
        want = rgb_cases.expected(m)
        assert np.array_equal(got[M:M + n], want), (name, i, m["width"], m["height"], m["rows"], m["plane_pitch"], m["rgb_pitch"], int((got[M:M + n] != want).sum()))


@pytest.mark.parametrize("layout", list(rgb_cases.LAYOUTS))
def test_every_width_height_and_pitch_equals_the_definition(gpu_codec, tables, layout):
    mine = [(n, t) for n, t in tables if n in ["%s %s" % (layout, p) for p in rgb_cases.PITCHES]]
    assert len(mine) == len(rgb_cases.PITCHES)
    for name, images in mine:
        check(gpu_codec.rgb(images), images, name)
    assert gpu_codec._L.lep_gpu_last_kernel_name(gpu_codec.handle) == b"lep_rgb_kernel"
    assert gpu_codec._L.lep_gpu_last_kernel_ms(gpu_codec.handle) > 0


def test_row_ranges(gpu_codec, tables):
    mine = [(n, t) for n, t in tables if "row ranges" in n]
    assert len(mine) == len(rgb_cases.LAYOUTS)
    for name, images in mine:
        assert {m["rows"] for m in images} >= {(5, 6), (3, 17), (0, 8), (8, 17), (9, 9)}
        check(gpu_codec.rgb(images), images, name)
    # two consecutive ranges: each writes its rows and nothing else, together they are the whole image
    name, images = mine[2]
    front = [m for m in images if m["rows"] == (0, 8) and m["width"] == rgb_cases.UNIT + 3][0]
    back = dict(front, rows=(8, 17))                        # the same planes
    a, b = gpu_codec.rgb([front])[0], gpu_codec.rgb([back])[0]
    cut = M + 8 * front["rgb_pitch"]
    both = np.frombuffer(a[:cut] + b[cut:], dtype=np.uint8)
    assert np.array_equal(both[M:-M], rgb_cases.expected(dict(front, rows=(0, 17))))


def test_images_of_different_geometry_in_one_launch(gpu_codec, tables):
    (name, images), = [(n, t) for n, t in tables if n == "mixed geometry"]
    check(gpu_codec.rgb(images), images, name)
    assert gpu_codec.rgb([]) == []


def refused(codec, images):
    with pytest.raises(LeptonError) as e:
        codec.rgb(images)
    assert e.value.code == 1, e.value                       # LEP_ASSERTION_FAILURE
    assert "lep_gpu_rgb_device" in str(e.value) and codec.last_error().startswith("lep_gpu_rgb_device: ")
    for buf in e.value.buffers:
        assert (np.frombuffer(buf, dtype=np.uint8) == rgb_cases.CANARY).all(), "a refused call wrote into an output"
    return codec.last_error()


def test_refusals_write_nothing(gpu_codec):
    rng = np.random.default_rng(3)
    good = [rgb_cases.image(rng, "420", 40, 17, "dwords"), rgb_cases.image(rng, "gray", 9, 5), rgb_cases.image(rng, "422", 259, 3)]
    check(gpu_codec.rgb(good), good)

    def broken(at, **change):
        images = copy.deepcopy(good)
        for k, v in change.items():
            images[at][k] = v(images[at][k]) if callable(v) else v
        return images

    assert "no plane" in refused(gpu_codec, broken(0, planes=lambda p: [p[0], None, p[2]]))
    assert "no output" in refused(gpu_codec, broken(2, no_output=True))
    assert "pitch" in refused(gpu_codec, broken(0, plane_pitch=lambda p: [p[0], 19, p[2]]))          # dw = 20
    assert "pitch" in refused(gpu_codec, broken(2, plane_pitch=lambda p: [258, p[1], p[2]]))
    assert "rgb_pitch" in refused(gpu_codec, broken(0, rgb_pitch=119))                               # 40 pixels: 120 bytes
    assert "rgb_pitch" in refused(gpu_codec, broken(1, rgb_pitch=8))
    for rows in ((0, 18), (-1, 3), (5, 4)):
        assert "rows" in refused(gpu_codec, broken(0, rows=rows))
    two = broken(0, planes=lambda p: p[:2], h_samp=[2, 1], v_samp=[2, 1], plane_pitch=lambda p: p[:2])
    assert "components" in refused(gpu_codec, two)
    assert "components" in refused(gpu_codec, broken(1, ncomp=0))
    assert "components" in refused(gpu_codec, broken(0, ncomp=4))
    assert "sampling" in refused(gpu_codec, broken(0, h_samp=[3, 2, 1]))                             # 2 in 3: no integral factor
    assert "sampling" in refused(gpu_codec, broken(2, v_samp=[2, 3, 1]))
    assert "sampling" in refused(gpu_codec, broken(0, h_samp=[2, 0, 1]))
    assert "pixels" in refused(gpu_codec, broken(0, width=0))
    check(gpu_codec.rgb(good), good)
