"""The images of the pixel tests (test_rgb_emulation.py steps lep_rgb.h's lanes through them on the CPU, test_gpu_rgb.py runs them through
GpuCodec.rgb): every layout the definition tells apart, widths on both sides of the dw <= 2 rule and of a wavefront unit's 256 pixels,
heights of both parities, pitches that equal the row, run wider on dwords and run wider by an odd count (rows then start off a dword:
byte loads and byte stores), whole images and row ranges.  Planes are random bytes with 0 and 255 among them, exactly
(dh - 1) * pitch + dw bytes long.  expected() is tests/rgb_ref.py."""
import numpy as np

import rgb_ref

CANARY = 0xEE
UNIT = 256                                  # pixels of a wavefront unit (lep_rgb.h kUnitPixels)
# layout -> (h_samp, v_samp, convert)
LAYOUTS = {
    "444": ([1, 1, 1], [1, 1, 1], True),
    "422": ([2, 1, 1], [1, 1, 1], True),            # (2, 1): triangle along the row, replication up to dw = 2
    "420": ([2, 1, 1], [2, 1, 1], True),            # (2, 2)
    "440": ([1, 1, 1], [2, 1, 1], True),            # (1, 2): triangle down the column at any width
    "411": ([4, 1, 1], [1, 1, 1], True),            # fh = 4: replication
    "chromafine": ([1, 2, 2], [1, 2, 2], True),     # the luma is the upsampled component
    "mixed": ([2, 2, 1], [2, 1, 1], True),          # Cb (1, 2), Cr (2, 2) in one frame
    "tall": ([2, 1, 1], [4, 1, 1], True),           # (2, 4): replication both ways
    "rgb420": ([2, 1, 1], [2, 1, 1], False),        # components as they are: upsampled, not converted
    "gray": ([2], [2], True),                       # one component: fh = fv = 1 whatever its factors say
}
WIDTHS = [1, 2, 3, 4, 5, 7, 8, UNIT - 1, UNIT, UNIT + 1, UNIT + 3]
HEIGHTS = [1, 2, 3, 17]
PITCHES = ["tight", "dwords", "odd"]


def image(rng, layout, width, height, pitches="tight", rows=None):
    hs, vs, convert = LAYOUTS[layout]
    geo = rgb_ref.geometry(width, height, hs, vs)
    row = width * (1 if len(hs) == 1 else 3)
    pad = {"tight": lambda n: n, "dwords": lambda n: -(-n // 4) * 4 + 8, "odd": lambda n: (n + 3) | 1}[pitches]
    planes, arrays, pitch = [], [], []
    for dw, dh, _, _ in geo:
        p = pad(dw)
        buf = rng.integers(0, 256, (dh - 1) * p + dw, dtype=np.uint8)
        extreme = rng.integers(0, 8, buf.shape)
        buf[extreme == 0] = 0
        buf[extreme == 1] = 255
        full = np.zeros(dh * p, dtype=np.uint8)
        full[:len(buf)] = buf
        planes.append(buf.tobytes()); arrays.append(full.reshape(dh, p)[:, :dw]); pitch.append(p)
    return {"layout": layout, "width": width, "height": height, "h_samp": list(hs), "v_samp": list(vs), "convert": convert, "planes": planes,
            "arrays": arrays, "plane_pitch": pitch, "rgb_pitch": pad(row), "row_bytes": row, "rows": rows or (0, height)}


def expected(m, nbytes=None):
    """the output buffer of image m: rgb_pitch * height bytes (or its first nbytes), CANARY except in the pixels of the requested rows"""
    px = rgb_ref.pixels(m["arrays"], m["width"], m["height"], m["h_samp"], m["v_samp"], m["convert"])
    out = np.full((m["height"], m["rgb_pitch"]), CANARY, dtype=np.uint8)
    y0, y1 = m["rows"]
    out[y0:y1, :m["row_bytes"]] = px.reshape(m["height"], m["row_bytes"])[y0:y1]
    return out.reshape(-1)[:nbytes]


def tables(seed=11):
    """[(name, [images of one launch])]: per layout and kind of pitch every width and height in one table; row ranges; a mixed table"""
    rng = np.random.default_rng(seed)
    out = []
    for layout in LAYOUTS:
        for pitches in PITCHES:
            out.append(("%s %s" % (layout, pitches), [image(rng, layout, w, h, pitches) for w in WIDTHS for h in HEIGHTS]))
    for layout in LAYOUTS:
        ranged = []
        for w, pitches in ((UNIT + 3, "tight"), (7, "odd"), (40, "dwords")):
            for rows in ((5, 6), (0, 1), (16, 17), (3, 17), (0, 8), (8, 17), (9, 9)):      # a single row, an odd start, both halves, an empty one
                ranged.append(image(rng, layout, w, 17, pitches, rows))
        out.append(("%s row ranges" % layout, ranged))
    out.append(("mixed geometry", [image(rng, "420", 259, 17), image(rng, "gray", 5, 3, "odd"), image(rng, "444", 300, 2, "dwords", (1, 1)),
                                   image(rng, "411", 33, 39, "dwords", (7, 30)), image(rng, "mixed", 299, 39, "odd"), image(rng, "440", 1, 1)]))
    return out


def units(m):
    return (m["rows"][1] - m["rows"][0]) * (-(-m["width"] // UNIT))
