"""lep_decompress_rgb on the GPU, through GpuCodec.decompress_rgb: the .lep of the fixtures test_rgb_reference.py holds against libjpeg,
and of files PIL cannot read or that end early.  The pixels must equal tests/rgb_ref.py on the planes tests/samples_ref.py makes of the
frame the parser reads from the original file (truncated and sliced files: the frame GpuCodec.decode fills from the .lep), and PIL
again for the files of the CPU list; a damaged stream returns what decompress returns for it; a file of two components is refused;
decompress of the same files still gives the original bytes."""
import numpy as np
import pytest

import rgb_ref
import samples_ref
import slice_cases as sc
from conftest import golden
from lepton_amd.codec import JpegImage, LepFile, LeptonError
from test_rgb_reference import FIXTURES, NUMPY_ONLY, OUTSIDE_DOMAIN, colour_variant, pil_pixels

pytestmark = pytest.mark.gpu

FROM_THE_LEP = ["truncated", "prog_truncated_mid"]       # files that end inside their scan: the frame is what the decoder fills from the .lep


def pixels_of(res):
    a = np.frombuffer(res["pixels"], dtype=np.uint8).reshape(res["height"], res["pitch"])[:, :res["width"] * res["channels"]]
    return a if res["channels"] == 1 else a.reshape(res["height"], res["width"], 3)


def check_against_definition(codec, lep, jpg, desc):
    res = codec.decompress_rgb(lep)
    w, h, hs, vs = rgb_ref.frame_header(jpg)
    assert (res["width"], res["height"], res["channels"], res["pitch"]) == (w, h, 1 if len(hs) == 1 else 3, w * (1 if len(hs) == 1 else 3))
    got, want = pixels_of(res), rgb_ref.pixels_of_file(jpg, samples_ref.planes_of(desc))
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    assert codec._L.lep_gpu_last_kernel_name(codec.handle) == b"lep_rgb_kernel"
    return got


@pytest.mark.parametrize("name", FIXTURES + OUTSIDE_DOMAIN + NUMPY_ONLY)
def test_whole_files(gpu_codec, name):
    jpg, lep = golden(name)
    img = JpegImage(jpg)
    got = check_against_definition(gpu_codec, lep, jpg, img.desc)
    if name in FIXTURES:
        assert np.array_equal(got, pil_pixels(jpg))
    assert gpu_codec.decompress(lep) == jpg


@pytest.mark.parametrize("kind", ["adobe0", "adobe1", "ids_rgb"])
def test_the_colour_space_rule_is_read_from_the_lep(gpu_codec, kind):
    jpg = colour_variant(golden("c444_96x80")[0], kind)
    lep = gpu_codec.compress(jpg)
    img = JpegImage(jpg)
    got = check_against_definition(gpu_codec, lep, jpg, img.desc)
    assert np.array_equal(got, pil_pixels(jpg))
    assert gpu_codec.decompress(lep) == jpg


def never_coded_blocks(frames):
    return sum(int((~fr.any(axis=2)).sum()) for fr in frames)


@pytest.mark.parametrize("name", FROM_THE_LEP)
def test_files_that_end_inside_their_scan(gpu_codec, name):
    jpg, lep = golden(name)
    f = LepFile(lep)
    gpu_codec.decode([f])
    check_against_definition(gpu_codec, lep, jpg, f.desc)
    assert never_coded_blocks(samples_ref.frames_of(f.desc)) > 0 or name != "truncated", "the sequential file's tail was coded after all"
    assert gpu_codec.decompress(lep) == jpg


def test_a_slice(gpu_codec):
    """a -startbyte / -trunc slice that starts inside the scan and ends inside it: the rows in front of it are what the definition
    makes of 128-valued samples -- grey"""
    layout = "420"
    jpg = sc.jpeg_of(layout)
    start, trunc, what = sc.positions(layout)[9]
    assert what == "trunc inside the scan, start in front of it"
    lep = gpu_codec.compress_slice(jpg, start, trunc)
    f = LepFile(lep)
    gpu_codec.decode([f])
    frames = samples_ref.frames_of(f.desc)
    assert not frames[0][0].any() and not frames[0][-1].any() and any(fr.any() for fr in frames)
    assert rgb_ref.converts(jpg)
    got = check_against_definition(gpu_codec, lep, jpg, f.desc)
    assert (got[:4] == 128).all() and (got != 128).any()
    assert gpu_codec.decompress(lep) == jpg[start:trunc]


def code_of(call):
    try:
        call()
        return 0
    except LeptonError as e:
        return e.code


def test_a_damaged_stream_returns_what_decompress_returns(gpu_codec):
    from test_decode_rows_emulation import damaged_case, damaged_stream

    img, _seg, stream = damaged_case((203, 149))
    codes = []
    for seed in range(10):
        lep = img.write_lep([damaged_stream(stream, seed)])
        want = code_of(lambda: gpu_codec.decompress(lep))
        assert code_of(lambda: gpu_codec.decompress_rgb(lep)) == want, seed
        codes.append(want)
    assert any(codes), "no damaged stream was refused"
    jpg, lep = golden("c444_96x80")      # a header that does not parse
    assert code_of(lambda: gpu_codec.decompress_rgb(lep[:40])) == code_of(lambda: gpu_codec.decompress(lep[:40])) != 0


def test_two_components_are_refused(gpu_codec):
    jpg, lep = golden("lay_two_components_120x40")
    with pytest.raises(LeptonError) as e:
        gpu_codec.decompress_rgb(lep)
    assert e.value.code == 42                               # LEP_UNSUPPORTED_JPEG
    assert gpu_codec.last_error().startswith("lep_decompress_rgb: ") and "components" in gpu_codec.last_error()
    assert gpu_codec.decompress(lep) == jpg
