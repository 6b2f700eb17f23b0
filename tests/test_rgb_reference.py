"""tests/rgb_ref.py (the numpy restatement of lep_rgb.h's definition: libjpeg's fancy upsampling and jdcolor's conversion) held against
libjpeg as PIL wraps it: the yardstick of the pixel tests.  Every file is parsed with lep_jpeg_open, its planes are made by
tests/samples_ref.py, and rgb_ref's pixels must equal PIL's .convert("RGB") (or "L") with zero differing bytes.  No GPU and no kernel
is involved."""
import io

import numpy as np
import pytest
from PIL import Image

import rgb_ref
import samples_ref
from conftest import golden
from lepton_amd.codec import JpegImage

# equal to libjpeg byte for byte
FIXTURES = ["c420_160x120", "c420_odd_203x149", "c422_128x72", "c444_96x80", "lay_440_97x50", "lay_chromafine_96x64", "lay_mixed_200x120",
            "one_block_8x8", "one_col_420_16x80", "one_col_8x64", "q100_64x64",
            # restart intervals, progressive, two segments, one component: the files of test_samples_reference.py
            "rst_c420_176x112", "prog_c420_320x240", "prog_c444_203x149", "prog_gray_120x88", "q30_256x256_4seg", "gray_120x88", "lay_gray22_80x56"]
# files PIL does not decode: rgb_ref alone, held to its shape and to the planes it was given
NUMPY_ONLY = ["lay_all22_64x48"]     # PIL: "broken data stream" (every component 2x2: libjpeg's MCU is 12 blocks, over its limit of 10)

# Generated files with a chroma frame outside the domain of the sample definition (samples_ref.in_domain is false for it; lep_samples.h:
# libjpeg's SIMD transform saturates between the passes there and differs from its own islow code).  The planes differ from libjpeg's
# in a few samples, so the pixels are held to libjpeg only where the upsampled components are libjpeg's; the test asserts the reason.
OUTSIDE_DOMAIN = ["lay_440_640x480_2seg", "seq_ycb_cr_422_640x480_2seg"]

WIDTHS = list(range(1, 10)) + [15, 16, 17, 33]
HEIGHTS = [1, 2, 3, 5, 17]


def pil_pixels(jpg):
    im = Image.open(io.BytesIO(jpg))
    return np.asarray(im.convert("L" if len(im.getbands()) == 1 else "RGB"))


def ref_pixels(jpg):
    img = JpegImage(jpg)
    return rgb_ref.pixels_of_file(jpg, samples_ref.planes_of(img.desc))


def differing(jpg):
    want, got = pil_pixels(jpg), ref_pixels(jpg)
    assert got is not None and got.shape == want.shape and got.dtype == np.uint8, (None if got is None else got.shape, want.shape)
    return int((got != want).sum())


@pytest.mark.parametrize("name", FIXTURES)
def test_definition_equals_libjpeg_on_the_fixtures(name):
    assert differing(golden(name)[0]) == 0


@pytest.mark.parametrize("name", NUMPY_ONLY)
def test_files_libjpeg_refuses_still_have_pixels(name):
    jpg = golden(name)[0]
    with pytest.raises(Exception):
        pil_pixels(jpg)
    w, h, hs, vs = rgb_ref.frame_header(jpg)
    img = JpegImage(jpg)
    planes = samples_ref.planes_of(img.desc)
    got = ref_pixels(jpg)
    assert got.shape == (h, w, 3) and len(set(zip(hs, vs))) == 1
    crops = [p[:h, :w] for p in planes]                                               # no component is upsampled
    assert np.array_equal(got, rgb_ref.ycc_to_rgb(*crops) if rgb_ref.converts(jpg) else np.stack(crops, axis=-1))


@pytest.mark.parametrize("name", OUTSIDE_DOMAIN)
def test_files_outside_the_sample_domain_equal_libjpeg_where_their_planes_do(name):
    jpg = golden(name)[0]
    img = JpegImage(jpg)
    assert not all(samples_ref.in_domain(f, list(img.desc.qtable_zigzag[c])) for c, f in enumerate(samples_ref.frames_of(img.desc)))
    w, h, hs, vs = rgb_ref.frame_header(jpg)
    planes = samples_ref.planes_of(img.desc)
    im = Image.open(io.BytesIO(jpg))
    im.draft("YCbCr", im.size)
    ycc = np.asarray(im)                    # libjpeg's components, upsampled and not converted
    assert im.mode == "YCbCr" and ycc.shape == (h, w, 3)
    ours = np.stack([rgb_ref.upsample(p[:dh, :dw], fh, fv)[:h, :w] for p, (dw, dh, fh, fv) in zip(planes, rgb_ref.geometry(w, h, hs, vs))], axis=-1)
    same = (ours == ycc).all(axis=-1)
    assert same.mean() > 0.999 and (ours[..., 0] == ycc[..., 0]).all()          # a few chroma samples, no luma sample
    want, got = pil_pixels(jpg), ref_pixels(jpg)
    assert np.array_equal(got[same], want[same])
    assert np.array_equal(rgb_ref.ycc_to_rgb(ycc[..., 0], ycc[..., 1], ycc[..., 2]), want)      # the conversion alone: everywhere


def generated(width, height, subsampling, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    base = np.stack([(xx * 37 + yy * 11) % 256, (xx * 5 + yy * 53) % 256, (xx * 23 + yy * 29 + 90) % 256], axis=-1)
    a = np.clip(base + rng.integers(-40, 41, base.shape), 0, 255).astype(np.uint8)
    out = io.BytesIO()
    Image.fromarray(a, "RGB").save(out, "JPEG", quality=90, subsampling=subsampling)
    return out.getvalue()


@pytest.mark.parametrize("subsampling", [0, 1, 2], ids=["444", "422", "420"])
def test_definition_equals_libjpeg_on_small_generated_files(subsampling):
    """widths and heights on both sides of the dw <= 2 rule, of both parities"""
    bad = []
    for w in WIDTHS:
        for h in HEIGHTS:
            n = differing(generated(w, h, subsampling, seed=w * 100 + h))
            if n:
                bad.append((w, h, n))
    assert not bad, bad


def segments(jpg):
    """[(marker, offset, total length)] of the marker segments in front of the first scan"""
    at, out = 2, []
    while jpg[at] == 0xFF:
        m, n = jpg[at + 1], int.from_bytes(jpg[at + 2:at + 4], "big")
        out.append((m, at, 2 + n))
        if m == 0xDA:
            return out
        at += 2 + n
    raise AssertionError("no scan")


def adobe(transform):
    return b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00" + bytes([transform])


def colour_variant(jpg, kind):
    segs = segments(jpg)
    (m0, at0, n0), = [s for s in segs if s[0] == 0xE0]
    assert jpg[at0 + 4:at0 + 9] == b"JFIF\0" and not any(s[0] == 0xEE for s in segs)
    if kind in ("adobe0", "adobe1"):
        return jpg[:at0] + adobe(int(kind[-1])) + jpg[at0 + n0:]
    out = bytearray(jpg)
    for m, at, n in segs:
        if m in (0xC0, 0xC1, 0xC2):
            for k in range(3):
                out[at + 4 + 6 + 3 * k] = b"RGB"[k]
        if m == 0xDA:
            for k in range(3):
                out[at + 4 + 1 + 2 * k] = b"RGB"[k]
    return bytes(out[:at0] + out[at0 + n0:])


@pytest.mark.parametrize("kind,converted", [("adobe0", False), ("adobe1", True), ("ids_rgb", False)])
def test_colour_space_rule_on_variants_of_one_file(kind, converted):
    jpg = golden("c444_96x80")[0]
    assert rgb_ref.converts(jpg)
    v = colour_variant(jpg, kind)
    assert rgb_ref.converts(v) == converted
    assert differing(v) == 0
    assert (pil_pixels(v) != pil_pixels(jpg)).any() != converted      # the rule shows in libjpeg's own pixels


Y_VALUES = [0, 1, 127, 128, 254, 255]


def test_colour_formulas_against_a_per_pixel_loop():
    cr, cb = np.mgrid[0:256, 0:256]
    rng = np.random.default_rng(5)

    def one(y, b, r):
        fix = rgb_ref.FIX
        b, r = b - 128, r - 128
        clamp = lambda v: min(max(v, 0), 255)
        return [clamp(y + ((fix(1.40200) * r + 32768) >> 16)), clamp(y + ((-fix(0.34414) * b + 32768 - fix(0.71414) * r) >> 16)),
                clamp(y + ((fix(1.77200) * b + 32768) >> 16))]

    assert [rgb_ref.FIX(f) for f in (1.40200, 1.77200, 0.34414, 0.71414)] == [91881, 116130, 22554, 46802]
    for y in Y_VALUES:
        got = rgb_ref.ycc_to_rgb(np.full((256, 256), y), cb, cr)
        assert got.shape == (256, 256, 3)
        picks = rng.choice(65536, 4096, replace=False)
        corners = np.array([0, 255, 255 * 256, 65535, 128 * 256 + 128])
        for at in np.concatenate([corners, picks]):
            r_, b_ = int(at) >> 8, int(at) & 255
            assert got[r_, b_].tolist() == one(y, b_, r_), (y, b_, r_)


@pytest.mark.parametrize("y", Y_VALUES)
def test_colour_conversion_equals_libjpeg_over_the_chroma_square(y):
    cr, cb = np.mgrid[0:256, 0:256]
    ycc = np.stack([np.full((256, 256), y), cb, cr], axis=-1).astype(np.uint8)
    out = io.BytesIO()
    Image.fromarray(ycc, "YCbCr").save(out, "JPEG", quality=100, subsampling=0)
    jpg = out.getvalue()
    img = JpegImage(jpg)
    planes = samples_ref.planes_of(img.desc)
    assert np.ptp(planes[1]) > 240 and np.ptp(planes[2]) > 240      # the decoded planes still span the square
    assert differing(jpg) == 0
