"""The definition of lep_gpu_rgb_device's arithmetic (lepton_amd/csrc/lep_rgb.h) restated in numpy with 64-bit integers: libjpeg's
default full-scale path from sample planes to pixels -- fancy upsampling, no merged upsampling, jdcolor's table arithmetic.
test_rgb_reference.py holds this file against libjpeg (PIL); the emulation and GPU tests hold the kernel against this file."""
import numpy as np


def FIX(f):
    return int(f * 65536 + 0.5)


def geometry(width, height, h_samp, v_samp):
    """per component (dw, dh, fh, fv); None where a factor does not divide the largest.  One component: fh = fv = 1 whatever it says"""
    n = len(h_samp)
    if n == 1:
        return [(width, height, 1, 1)]
    hmax, vmax = max(h_samp), max(v_samp)
    if any(hmax % h for h in h_samp) or any(vmax % v for v in v_samp):
        return None
    return [(-(-width * h // hmax), -(-height * v // vmax), hmax // h, vmax // v) for h, v in zip(h_samp, v_samp)]


def _left(a):
    return np.concatenate([a[:, :1], a[:, :-1]], axis=1)


def _right(a):
    return np.concatenate([a[:, 1:], a[:, -1:]], axis=1)


def upsample(x, fh, fv):
    """x: (dh, dw) samples -> (dh * fv, dw * fh) int64, not cropped"""
    x = np.asarray(x).astype(np.int64)
    dh, dw = x.shape
    if (fh, fv) == (1, 1):
        return x
    up = np.concatenate([x[:1], x[:-1]], axis=0)
    dn = np.concatenate([x[1:], x[-1:]], axis=0)
    if (fh, fv) == (1, 2):
        out = np.empty((dh * 2, dw), dtype=np.int64)
        out[0::2] = (3 * x + up + 1) >> 2
        out[1::2] = (3 * x + dn + 2) >> 2
        return out
    if (fh, fv) == (2, 1) and dw > 2:
        out = np.empty((dh, dw * 2), dtype=np.int64)
        out[:, 0::2] = (3 * x + _left(x) + 1) >> 2
        out[:, 1::2] = (3 * x + _right(x) + 2) >> 2
        return out
    if (fh, fv) == (2, 2) and dw > 2:
        s = np.empty((dh * 2, dw), dtype=np.int64)
        s[0::2] = 3 * x + up
        s[1::2] = 3 * x + dn
        out = np.empty((dh * 2, dw * 2), dtype=np.int64)
        out[:, 0::2] = (3 * s + _left(s) + 8) >> 4
        out[:, 1::2] = (3 * s + _right(s) + 7) >> 4
        return out
    return np.repeat(np.repeat(x, fv, axis=0), fh, axis=1)


def ycc_to_rgb(y, cb, cr):
    """three int64 arrays of one shape -> (..., 3) uint8"""
    y, cb, cr = (np.asarray(a).astype(np.int64) for a in (y, cb, cr))
    cb, cr = cb - 128, cr - 128
    r = y + ((FIX(1.40200) * cr + 32768) >> 16)
    b = y + ((FIX(1.77200) * cb + 32768) >> 16)
    g = y + ((-FIX(0.34414) * cb + 32768 - FIX(0.71414) * cr) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def pixels(planes, width, height, h_samp, v_samp, convert=True):
    """planes: per component a 2-D uint8 array that holds at least the component's dw x dh samples at its top left (a block grid does)
    -> (height, width, 3) uint8, or (height, width) for one component; None for an image the entry point refuses"""
    if len(planes) not in (1, 3):
        return None
    geo = geometry(width, height, list(h_samp), list(v_samp))
    if geo is None:
        return None
    full = []
    for p, (dw, dh, fh, fv) in zip(planes, geo):
        p = np.asarray(p)
        assert p.shape[0] >= dh and p.shape[1] >= dw, (p.shape, dw, dh)
        full.append(upsample(p[:dh, :dw], fh, fv)[:height, :width])
    if len(full) == 1:
        return full[0].astype(np.uint8)
    if convert:
        return ycc_to_rgb(*full)
    return np.stack(full, axis=-1).astype(np.uint8)


def frame_header(jpg):
    """(width, height, h_samp, v_samp) of the file's first frame header"""
    jpg = bytes(jpg)
    at = 2
    while at + 4 <= len(jpg) and jpg[at] == 0xFF:
        m, n = jpg[at + 1], int.from_bytes(jpg[at + 2:at + 4], "big")
        if m in (0xC0, 0xC1, 0xC2):
            b = jpg[at + 4:at + 2 + n]
            nc = b[5]
            return (int.from_bytes(b[3:5], "big"), int.from_bytes(b[1:3], "big"), [b[7 + 3 * k] >> 4 for k in range(nc)], [b[7 + 3 * k] & 15 for k in range(nc)])
        at += 2 + n
    raise ValueError("no frame header")


def pixels_of_file(jpg, planes):
    """pixels() with the geometry and the colour rule read from the file's own headers"""
    w, h, hs, vs = frame_header(jpg)
    return pixels(planes, w, h, hs, vs, converts(jpg))


def converts(jpg):
    """libjpeg's rule for a three-component file, from the marker segments in front of the first scan and the frame's component ids:
    True = the components are Y, Cb, Cr.  JFIF APP0 -> yes; else Adobe APP14: transform 0 -> no, anything else -> yes; else the ids
    'R', 'G', 'B' -> no; else yes"""
    jpg = bytes(jpg)
    at, jfif, adobe, ids = 2, False, None, []
    while at + 4 <= len(jpg) and jpg[at] == 0xFF:
        m, n = jpg[at + 1], int.from_bytes(jpg[at + 2:at + 4], "big")
        body = jpg[at + 4:at + 2 + n]
        if m == 0xE0 and n >= 2 + 14 and body[:5] == b"JFIF\0":
            jfif = True
        if m == 0xEE and n >= 2 + 12 and body[:5] == b"Adobe":
            adobe = body[11]
        if m in (0xC0, 0xC1, 0xC2):
            ids = [body[6 + 3 * k] for k in range(body[5])]
        if m == 0xDA:
            break
        at += 2 + n
    if jfif:
        return True
    if adobe is not None:
        return adobe != 0
    return ids != [ord("R"), ord("G"), ord("B")]
