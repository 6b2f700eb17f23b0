"""The definition of lep_gpu_samples_device's arithmetic (lepton_amd/csrc/lep_samples.h) restated in numpy with 64-bit integers, and
helpers that build planes from coefficient frames.  test_samples_reference.py holds this file against libjpeg (PIL); the emulation and
GPU tests hold the kernels against this file."""
import ctypes as C

import numpy as np

# raster index of aligned entry a (lep_core.h kA2R) and of zig-zag entry z
A2R = np.array([9, 10, 17, 25, 18, 11, 12, 19, 26, 33, 41, 34, 27, 20, 13, 14, 21, 28, 35, 42, 49, 57, 50, 43, 36,
                29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63,
                0, 1, 2, 3, 4, 5, 6, 7, 8, 16, 24, 32, 40, 48, 56])
Z2R = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34,
                27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
DC_ALIGNED = 49


def idct_pass(x):
    """one pass over the last axis (8 values), not descaled"""
    i0, i1, i2, i3, i4, i5, i6, i7 = (x[..., k] for k in range(8))
    z1 = (i2 + i6) * 4433
    t2 = z1 - i6 * 15137
    t3 = z1 + i2 * 6270
    t0 = (i0 + i4) << 13
    t1 = (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i7, i5, i3, i1
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    return np.stack([t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3], axis=-1)


def descale(x, s):
    return (x + (1 << (s - 1))) >> s


def dequantised(frame, q_zigzag):
    """frame: (rows, cols, 64) int16 in aligned order -> (rows, cols, 8, 8) int64 rasters of d = c * q"""
    q = np.zeros(64, dtype=np.int64)
    q[Z2R] = np.asarray(q_zigzag, dtype=np.int64)
    d = np.zeros(frame.shape, dtype=np.int64)
    d[..., A2R] = frame.astype(np.int64)
    return (d * q).reshape(frame.shape[0], frame.shape[1], 8, 8)


def between_passes(frame, q_zigzag):
    """the values between the column pass and the row pass (the domain bounds them by 32767)"""
    d = dequantised(frame, q_zigzag)
    return descale(idct_pass(d.swapaxes(-1, -2)), 11).swapaxes(-1, -2)


def in_domain(frame, q_zigzag):
    return int(np.abs(dequantised(frame, q_zigzag)).max(initial=0)) <= 32767 and int(np.abs(between_passes(frame, q_zigzag)).max(initial=0)) <= 32767


def plane(frame, q_zigzag, scale=1):
    """frame: (rows, cols, 64) int16, aligned order -> (rows * 8 / scale, cols * 8 / scale) uint8"""
    rows, cols = frame.shape[:2]
    if scale == 8:
        dc = frame[..., DC_ALIGNED].astype(np.int64) * int(q_zigzag[0])
        return np.clip(((dc + 4) >> 3) + 128, 0, 255).astype(np.uint8)
    assert scale == 1
    out = descale(idct_pass(between_passes(frame, q_zigzag)), 18)          # (rows, cols, y, x)
    return np.clip(out + 128, 0, 255).astype(np.uint8).transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8)


def frames_of(desc):
    """the coefficient frames of an ImageDesc with host pointers (JpegImage.desc, LepFile.desc after GpuCodec.decode), copied"""
    out = []
    for c in range(desc.ncomp):
        w, h = desc.width_blocks[c], desc.height_blocks[c]
        raw = C.string_at(desc.blocks[c], w * h * 128)
        out.append(np.frombuffer(raw, dtype=np.int16).reshape(h, w, 64).copy())
    return out


def planes_of(desc, scale=1):
    """every component's plane from an ImageDesc with host pointers"""
    return [plane(f, list(desc.qtable_zigzag[c]), scale) for c, f in enumerate(frames_of(desc))]
