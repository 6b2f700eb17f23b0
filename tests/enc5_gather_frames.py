"""Frames for the tests of the split-phase encoder's gather pass (lep_enc5.h Walk5::put_bin / drain / flush_bin): quantised coefficients
written into the descriptor of a corpus.synth_jpeg file, chosen for what they do to the lanes' staging of bins -- not for what they show.
Aligned coefficient order: 0..48 the 7x7 interior, 49 the DC, 50..63 the two edges."""
import ctypes as C
import io

import numpy as np

from lepton_amd import corpus
from lepton_amd.codec import JpegImage

CONTENTS = ("dense", "one_per_block", "alternating", "empty_beside_dense")


# raster place (8 * vertical + horizontal frequency) of the coefficient at each aligned place (lep_core.h kA2R)
A2R = np.array([9, 10, 17, 25, 18, 11, 12, 19, 26, 33, 41, 34, 27, 20, 13, 14, 21, 28, 35, 42, 49, 57, 50, 43, 36,
                29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
                0, 1, 2, 3, 4, 5, 6, 7, 8, 16, 24, 32, 40, 48, 56])


def _dense(rng, nb, w):
    """every coefficient +-1024..2047: 22 bins per coefficient, threshold units on the edges, a large DC delta -- the most a lane can put
    between two check points, and two complete sectors in one lane.  Pixels of such blocks swing by thousands, and a DC predicted from
    a neighbour's border that far off is one the coder refuses (exit code 6); so the blocks are ONE random block mirrored from
    neighbour to neighbour (odd horizontal frequencies negated in odd columns, odd vertical ones in odd rows): every border is
    continuous and the prediction is the neighbours' DC."""
    base = rng.integers(1024, 2048, 64) * rng.choice([-1, 1], 64)
    b = np.arange(nb)
    flip = ((A2R & 7)[None, :] * (b % w)[:, None] + (A2R >> 3)[None, :] * (b // w)[:, None]) & 1
    v = base[None, :] * (1 - 2 * flip)
    v[:, 49] = rng.integers(-1000, 1001, nb)
    return v


def _one(rng, nb):
    """one +-1 per block: a lane needs many rows for a sector while nothing is urgent"""
    v = np.zeros((nb, 64), dtype=np.int64)
    at = rng.integers(0, 63, nb)
    at[at >= 49] += 1   # (not the DC)
    v[np.arange(nb), at] = rng.choice([-1, 1], nb)
    return v


def _empty(rng, nb):
    """nothing but a small DC: an interior run of the six count bins, an edge run of six count bins and the DC's"""
    v = np.zeros((nb, 64), dtype=np.int64)
    v[:, 49] = rng.integers(-1, 2, nb)
    return v


def coefficients(content, c, nb, w):
    """nb blocks of component c, w to the row"""
    rng = np.random.default_rng(100 * CONTENTS.index(content) + c)
    if content == "dense":
        return _dense(rng, nb, w)
    if content == "one_per_block":
        return _one(rng, nb)
    # Beside a flat block no mirroring helps: the prediction is off by the dense block's border, and with coefficients of 11 bits the
    # reference coder refuses the frame (exit code 6).  The dense blocks of the mixed frames therefore hold +-128..255 -- 17 bins per
    # coefficient, still half a sector -- and no DC; the 25-bins bound is the dense frame's business.
    v = rng.integers(128, 256, (nb, 64)) * rng.choice([-1, 1], (nb, 64))
    v[:, 49] = 0
    if content == "alternating":           # the lanes maximally out of phase
        v[1::2] = _one(rng, nb)[1::2]
    else:                                   # short runs that start and end inside a sector shared with dense neighbours
        v[1::3] = _empty(rng, nb)[1::3]
        v[5::7, :49] = 0                   # ... and interiors that are empty beside full edges
    return v


def _jpeg(w_blocks, h_blocks, gray):
    jpg = corpus.synth_jpeg(8 * w_blocks, 8 * h_blocks, 31, quality=100)
    if not gray:
        return jpg
    from PIL import Image

    buf = io.BytesIO()
    Image.open(io.BytesIO(jpg)).convert("L").save(buf, format="JPEG", quality=100, optimize=False)
    return buf.getvalue()


def frame(w_blocks, h_blocks, gray, content):
    """a JpegImage of w_blocks x h_blocks luma blocks (4:2:0 rounds both up to even), one component or three, filled with `content`"""
    img = JpegImage(_jpeg(w_blocks, h_blocks, gray))
    d = img.desc
    assert d.ncomp == (1 if gray else 3)
    for c in range(d.ncomp):
        n = d.nblocks(c)
        a = np.frombuffer((C.c_int16 * (n * 64)).from_address(d.blocks[c]), dtype=np.int16)
        a[:] = coefficients(content, c, n, d.width_blocks[c]).ravel()
    return img


# (luma blocks per row, block rows, one component): rows of 1, 63, 64, 65 and 129 blocks -- less than a tile, a tile but one, a tile, a
# tile and one, two tiles and one -- of 2 to 4 block rows
SHAPES = [(1, 4, False), (63, 2, False), (64, 4, False), (65, 2, False), (129, 4, False),
          (1, 3, True), (63, 3, True), (64, 2, True), (65, 3, True), (129, 4, True)]
