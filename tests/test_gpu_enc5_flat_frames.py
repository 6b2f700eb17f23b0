"""Flat frames through the whole encoder on the MI355X.  A solid-colour JPEG is one thread segment of some hundred thousand bins that
all but repeat -- 1024x1024 at quality 90: 319,532 bins in a 349-byte stream -- and on such a list two runs of the bool writer's range
recurrence never fall into step: the stitched writer's link pass (lep_enc5.h wchunk_link_cuts) finds nearly every chunk's guessed start
range wrong and runs the chunk's range again, and most chunks start before or inside the few bytes the stream has.  Frames of photographs
never do that.  Here: a solid red and a solid grey file, a frame of all-zero coefficients and one synthetic photograph (which does fall
into step), each alone and all in one launch, through the default codec, the stitched writer at 64 and at 4 chunks, the writer in part
chunks beside gather at 8 x 4, the lane-per-segment writer and the single-kernel encoder: streams are the oracle's, the device decoder
returns the frames, and the writer's records (lep_gpu_debug_wchunks) show that the redo branch ran.  Wrong guesses seen on the MI355X,
alone and in the launch of all four: at 64 chunks 60 of 63 for the red file, 62 for the grey one, 32 .. 39 for each of the zero frame's
eight segments, 0 for the photograph's four; at 4 chunks 3 of 3, 3, 2, 0; at 8 parts x 4 chunks 30 of 31, 31, 16 .. 20, 0.
Then reservations too small, through lep_gpu_encode_device: status 100 for exactly the segments whose reservation is short of the
oracle's length, the others' streams intact beside them, the guard bytes around the arena untouched."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import bool_writer_ref as bw
import oracle_binding as ob
from enc5_gather_frames import frame
from lepton_amd import abi, corpus
from lepton_amd.codec import GpuCodec, JpegImage, LepFile

KNOBS = ("LEP_ENC5_MIN", "LEP_ENC5_WCHUNKS", "LEP_ENC5_WMAXSEG", "LEP_ENC5_WSCHED", "LEP_ENC5_PARTS", "LEP_ENC5_WPARTCHUNKS", "LEP_ENC_WAVES")
CODECS = {
    "default": {},
    "stitched_64_chunks": {"LEP_ENC5_MIN": "1", "LEP_ENC5_WCHUNKS": "64"},
    "stitched_4_chunks": {"LEP_ENC5_MIN": "1", "LEP_ENC5_WCHUNKS": "4"},
    "lane_per_segment": {"LEP_ENC5_MIN": "1", "LEP_ENC5_WCHUNKS": "0"},
    "beside_8_parts_4_chunks": {"LEP_ENC5_MIN": "1", "LEP_ENC5_WMAXSEG": "0", "LEP_ENC5_WSCHED": "beside", "LEP_ENC5_PARTS": "8", "LEP_ENC5_WPARTCHUNKS": "4"},
    "single_kernel": {"LEP_ENC5_MIN": "0"},
}
CHUNKED = {"stitched_64_chunks": (1, 64), "stitched_4_chunks": (1, 4), "beside_8_parts_4_chunks": (8, 4)}   # (parts, chunks) of their records
GUARD, GAP = 0x5C, 256
CASES = {}


def solid_jpeg(w, h, colour):
    from PIL import Image

    buf = io.BytesIO()
    Image.new("RGB", (w, h), colour).save(buf, format="JPEG", quality=90)
    return buf.getvalue()


def zero_frame():
    img = frame(128, 128, False, "one_per_block")
    for c in range(img.desc.ncomp):
        C.memset(img.desc.blocks[c], 0, img.desc.nblocks(c) * 128)
    return img


def case(img, plan=None):
    plan = plan or img.plan()
    want, _ = ob.oracle_encode(img.desc, plan)
    d = img.desc
    return img, plan, want, [C.string_at(d.blocks[c], d.coded_blocks[c] * 128) for c in range(d.ncomp)]


def flat_cases():
    """once: {name: (image, plan, oracle streams, frame bytes)}"""
    if "flat" not in CASES:
        CASES["jpegs"] = {"red": solid_jpeg(1024, 1024, (200, 30, 30)), "grey": solid_jpeg(2048, 1024, (128, 128, 128))}
        CASES["flat"] = {"red": case(JpegImage(CASES["jpegs"]["red"])), "grey": case(JpegImage(CASES["jpegs"]["grey"])), "zero": case(zero_frame()),
                         "synth": case(JpegImage(corpus.synth_jpeg(1024, 1024, 7)))}
        assert len(CASES["flat"]["red"][1]) == 1 and len(CASES["flat"]["grey"][1]) == 1   # (one thread segment each: 349 and 655 bytes)
    return CASES["flat"]


@pytest.fixture(scope="module", params=list(CODECS), ids=list(CODECS))
def codec(request):
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(CODECS[request.param])
    try:
        c = GpuCodec(0)
        c.flat_name = request.param
        return c
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def wrong_guesses(codec, nseg):
    """per segment of the launch just made: chunks whose guessed start range the link pass found wrong"""
    parts, chunks, recs = codec.debug_wchunks()
    assert (parts, chunks) == CHUNKED[codec.flat_name] and recs.shape[0] == nseg, (parts, chunks, None if recs is None else recs.shape)
    return [bw.chunk_counts(recs[s])[0] for s in range(nseg)]


def check_redo(codec, names, cases):
    """the redo branch ran on the solid files and not on the photograph"""
    if codec.flat_name not in CHUNKED:
        return
    wrong, at = wrong_guesses(codec, sum(len(cases[n][1]) for n in names)), 0
    print(codec.flat_name, "+".join(names), "wrong guesses per segment:", wrong)
    for n in names:
        mine = wrong[at:at + len(cases[n][1])]
        at += len(mine)
        if n in ("red", "grey"):
            assert mine[0] >= (32 if CHUNKED[codec.flat_name] == (1, 64) else 1), (n, mine)
        if n == "synth":
            assert mine == [0] * len(mine), (n, mine)


@pytest.mark.gpu
@pytest.mark.parametrize("names", [("red",), ("grey",), ("zero",), ("synth",), ("red", "grey", "zero", "synth")], ids=["red", "grey", "zero", "synth", "together"])
def test_gpu_flat_frames_equal_the_oracle(codec, names):
    cases = flat_cases()
    got = codec.encode([cases[n][0] for n in names], [cases[n][1] for n in names])
    kernel = codec._L.lep_gpu_last_kernel_name(codec.handle)
    if codec.flat_name not in ("default", "single_kernel"):
        assert b"enc5" in kernel and (b"beside gather" in kernel) == (codec.flat_name == "beside_8_parts_4_chunks"), kernel
    if codec.flat_name == "single_kernel":
        assert b"enc5" not in kernel, kernel
    for n, streams in zip(names, got):
        want = cases[n][2]
        assert [len(s) for s in streams] == [len(w) for w in want], n
        assert streams == want, n
    check_redo(codec, names, cases)


@pytest.mark.gpu
def test_gpu_flat_frames_decode_to_the_frames(codec):
    cases = flat_cases()
    files = [LepFile(img.write_lep(want)) for img, _, want, _ in cases.values()]
    codec.decode(files)
    for f, (_, _, _, fr) in zip(files, cases.values()):
        for c in range(f.desc.ncomp):
            assert C.string_at(f.desc.blocks[c], len(fr[c])) == fr[c]


@pytest.mark.gpu
def test_gpu_solid_files_round_trip(gpu_codec):
    flat_cases()
    for name, jpg in CASES["jpegs"].items():
        lep = gpu_codec.compress(jpg)
        assert len(lep) < len(jpg) // 4, name
        assert gpu_codec.decompress(lep) == jpg, name


def split(img, n):
    """n thread segments of about equal height, cut on even luma block rows"""
    h = img.desc.height_blocks[0]
    step = max(2, (h // n) & ~1)
    ys = list(range(0, h, step))[:n]
    return [abi.Segment(0, y, ys[k + 1] if k + 1 < len(ys) else h, 1 if k + 1 == len(ys) else 0) for k, y in enumerate(ys)]


def small_cases():
    """once: a solid file in 4 segments, a dense frame in 6, a photograph in 4"""
    if "small" not in CASES:
        imgs = [JpegImage(solid_jpeg(256, 256, (200, 30, 30))), frame(65, 12, False, "dense"), JpegImage(corpus.synth_jpeg(256, 192, 7))]
        CASES["small"] = [case(img, split(img, n)) for img, n in zip(imgs, (4, 6, 4))]
    return CASES["small"]


def encode_device(codec, cases, caps):
    """lep_gpu_encode_device into a guard-filled arena: reservation k holds caps[k] bytes, GAP guard bytes lie in front of the first and
    behind the last -> (arena, offsets, lengths, status)"""
    L, h = codec._L, codec.handle
    owned = []

    def dmalloc(n):
        p = C.c_void_p()
        assert L.lep_gpu_malloc(h, n, C.byref(p)) == 0
        owned.append(p)
        return p

    try:
        nimg = len(cases)
        descs = (abi.ImageDesc * nimg)(*[c[0].desc for c in cases])
        flat = []
        for i, (img, plan, _, _) in enumerate(cases):
            for c in range(img.desc.ncomp):
                p = dmalloc(img.desc.nblocks(c) * 128 + 256)
                assert L.lep_gpu_memcpy_h2d(h, p, img.desc.blocks[c], img.desc.nblocks(c) * 128) == 0
                descs[i].blocks[c] = p.value
            flat += [abi.Segment(i, s.luma_y_start, s.luma_y_end, s.is_last) for s in plan]
        nseg = len(flat)
        assert nseg == len(caps)
        segs = (abi.Segment * nseg)(*flat)
        offs = (C.c_uint64 * (nseg + 1))()
        offs[0] = GAP
        for k, cap in enumerate(caps):
            offs[k + 1] = offs[k] + cap
        size = offs[nseg] + GAP
        d_streams, d_len, d_status = dmalloc(size), dmalloc(4 * nseg), dmalloc(4 * nseg)
        assert L.lep_gpu_memset(h, d_streams, GUARD, size) == 0
        rc = L.lep_gpu_encode_device(h, descs, nimg, segs, nseg, d_streams, offs, d_len, d_status, None)
        assert rc == 0, (rc, codec.last_error())
        assert L.lep_gpu_sync(h) == 0, codec.last_error()
        arena, lens, status = np.zeros(size, dtype=np.uint8), np.zeros(nseg, dtype=np.uint32), np.zeros(nseg, dtype=np.int32)
        for dst, src in ((arena, d_streams), (lens, d_len), (status, d_status)):
            assert L.lep_gpu_memcpy_d2h(h, dst.ctypes.data_as(C.c_void_p), src, dst.nbytes) == 0
        return arena, list(offs), lens, status
    finally:
        for p in owned:
            L.lep_gpu_free(h, p)


@pytest.mark.gpu
def test_gpu_encoders_report_reservations_too_small_and_spare_the_neighbours(codec):
    """14 segments of three small frames; every third reservation is short of the oracle's length L by 2 bytes or by half, the others
    hold L + 2 or L + 40: status 100 for exactly the short ones, the others' streams are the oracle's"""
    cases = small_cases()
    want = [w for c in cases for w in c[2]]
    assert 8 <= len(want) <= 20
    short = [k % 3 == 2 for k in range(len(want))]
    caps = [(len(w) - 2 if k % 2 else len(w) // 2) if short[k] else len(w) + (2 if k % 2 else 40) for k, w in enumerate(want)]
    arena, offs, lens, status = encode_device(codec, cases, caps)
    kernel = codec._L.lep_gpu_last_kernel_name(codec.handle)
    assert (b"enc5" in kernel) == (codec.flat_name != "single_kernel"), kernel
    assert (arena[:GAP] == GUARD).all() and (arena[offs[-1]:] == GUARD).all() and len(arena) - offs[-1] == GAP
    for k, w in enumerate(want):
        if short[k]:
            assert status[k] == 100, (k, int(status[k]), caps[k], len(w))
        else:
            assert status[k] == 0 and lens[k] == len(w), (k, int(status[k]), int(lens[k]), len(w))
            assert bytes(arena[offs[k]:offs[k] + len(w)]) == w, k
