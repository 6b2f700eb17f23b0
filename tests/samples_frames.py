"""Coefficient frames shared by the sample-plane tests (the lane-by-lane emulation on the CPU and the kernels on the GPU).

A frame is (q, blocks): the quantisation table in zig-zag order (64 uint16) and the blocks, (rows, cols, 64) int16 in aligned order.

The domain (lep_samples.h): every |d[k]| = |c[k] * q[k]| <= 32767 and every value between the two passes <= 32767 in magnitude; there
32-bit arithmetic is exact and the kernels must equal tests/samples_ref.py, which computes in 64 bits.  in_domain frames:
  - random frames of every width that takes another path through a unit of eight blocks (1, 7, 8, 9, 17 blocks; 1 and 3 block rows),
    dense, |d| <= 1000: a pass's output is a linear form whose absolute coefficients sum to at most 61214, so the values between the
    passes stay below 1000 * 61214 / 2048 = 29890;
  - the domain's corners.  A block whose 64 values are all +-32767 is NOT in the domain, whatever its signs: with the signs of one
    output's linear form the values between the passes reach 979394, and the second pass then leaves 32 bits (the 64-bit restatement
    and wrapping 32-bit arithmetic differ in 10 samples of such a block) -- those blocks are in outside_domain() below.  The corners
    that are in the domain, one block each:
      * a DC of +-32767 alone (the largest |d|; one term per sum, so nothing wraps);
      * all 64 values +-m with the signs of column output k's linear form (and with the outer product of the signs of column output
        k's and row output k2's), m the largest magnitude that keeps the values between the passes within 32767 (found with
        samples_ref.in_domain, 1096): the corner of the bound between the passes, every output and both signs;
      * the first row +-8191 with the signs of row output k's linear form, the rest zero: every value between the passes is
        +-32764, and the row pass sums 61214 * 32764 = 2.006e9, the nearest a sum inside the domain comes to 2^31.
outside_domain(): c = -32768 / 32767 with q = 65535, and the all-+-32767 blocks: no result is compared, only that nothing is read or
written out of bounds and that no signed arithmetic overflows."""
import numpy as np

import samples_ref

DC = samples_ref.DC_ALIGNED


def _forms():
    """M[k][j]: coefficient of input j in output k of one pass"""
    return np.stack([samples_ref.idct_pass(np.eye(8, dtype=np.int64)[j]) for j in range(8)], axis=1)


def _frame_of_rasters(rasters, cols):
    """blocks given as 8x8 rasters of coefficients -> a frame `cols` blocks wide, zero blocks at the end of the last row"""
    rows = (len(rasters) + cols - 1) // cols
    f = np.zeros((rows * cols, 64), dtype=np.int16)
    for i, r in enumerate(rasters):
        f[i] = np.asarray(r, dtype=np.int64).reshape(64)[samples_ref.A2R]
    return f.reshape(rows, cols, 64)


def random_frame(cols, rows, seed):
    rng = np.random.default_rng(seed)
    q = rng.integers(1, 65, 64).astype(np.uint16)
    q_raster = np.zeros(64, dtype=np.int64)
    q_raster[samples_ref.Z2R] = q
    q_aligned = q_raster[samples_ref.A2R]
    lim = 1000 // q_aligned
    blocks = rng.integers(-lim, lim + 1, (rows, cols, 64)).astype(np.int16)
    return q, blocks


def all_signs_blocks(magnitude):
    """all 64 values +-magnitude: the signs of column output k's form in every column (both signs), and the outer products with row output k2's"""
    S = np.where(_forms() >= 0, 1, -1)
    out = []
    for k in range(8):
        for sgn in (1, -1):
            out.append(np.tile((sgn * S[k] * magnitude)[:, None], (1, 8)))
        for k2 in range(8):
            out.append(np.outer(S[k], S[k2]) * magnitude)
    return out


def corner_frame():
    S = np.where(_forms() >= 0, 1, -1)
    q = np.ones(64, dtype=np.uint16)
    m = 1200
    while not samples_ref.in_domain(_frame_of_rasters(all_signs_blocks(m), 9), q):
        m -= 1
    assert m == 1096, m
    rasters = []
    for sgn in (1, -1):
        r = np.zeros((8, 8), dtype=np.int64)
        r[0, 0] = sgn * 32767
        rasters.append(r)
    rasters += all_signs_blocks(m)
    for k in range(8):
        for sgn in (1, -1):
            r = np.zeros((8, 8), dtype=np.int64)
            r[0, :] = sgn * S[k] * 8191
            rasters.append(r)
    return q, _frame_of_rasters(rasters, 9)


def corner_frame_with_table():
    """the DC corner reached through the table: 32767 = 7 * 4681"""
    q = np.full(64, 7, dtype=np.uint16)
    f = np.zeros((1, 2, 64), dtype=np.int16)
    f[0, 0, DC], f[0, 1, DC] = 4681, -4681
    return q, f


def in_domain():
    """[(name, q, blocks)]"""
    out = [("random_%dx%d" % (c, r), *random_frame(c, r, 100 * c + r)) for c in (1, 7, 8, 9, 17) for r in (1, 3)]
    out.append(("corners", *corner_frame()))
    out.append(("dc_corner_q7", *corner_frame_with_table()))
    for name, q, f in out:
        # (the DC corners are the one place where a value between the passes exceeds 32767: 4 * 32767, a single term)
        assert name.startswith("dc_corner") or name == "corners" or samples_ref.in_domain(f, q), name
    return out


def outside_domain():
    rng = np.random.default_rng(5)
    q = np.full(64, 65535, dtype=np.uint16)
    far = np.where(rng.integers(0, 2, (3, 9, 64)) == 1, 32767, -32768).astype(np.int16)
    return [("far_outside", q, far), ("all_32767", np.ones(64, dtype=np.uint16), _frame_of_rasters(all_signs_blocks(32767), 9))]


CANARY = 0xEE


def plane_size(blocks, scale):
    """(height, width) in samples of the plane of a frame"""
    return blocks.shape[0] * 8 // scale, blocks.shape[1] * 8 // scale


def expected_rows(q, blocks, scale, rows, pitch):
    """what a plane's buffer must hold after block rows [rows[0], rows[1]) were written into CANARY bytes: (height, pitch) uint8 -- the
    samples of those rows, CANARY in the other rows and in the pitch padding"""
    h, w = plane_size(blocks, scale)
    out = np.full((h, pitch), CANARY, dtype=np.uint8)
    per = 8 // scale
    if rows[1] > rows[0]:
        out[rows[0] * per:rows[1] * per, :w] = samples_ref.plane(blocks[rows[0]:rows[1]], list(q), scale)
    return out
