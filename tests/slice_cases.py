"""Files and slice positions shared by the slice tests (CPU and GPU): small baseline files of three layouts, written by
tests/jpeg_writer.py with fixed seeds, and for each the (start_byte, trunc) pairs `lepton -startbyte -trunc` is asked for -- drawn
from the file's own hand-off records so that every kind of position occurs: inside the header, exactly on a record's byte, one byte
on either side of it, in the last MCU row, behind the last row, trunc = 0, trunc inside the scan, trunc <= start_byte."""
import ctypes as C
import functools

import numpy as np

# name -> (width, height, [(component id, h, v, quantisation table, DC table, AC table)])
LAYOUTS = {
    "420": (128, 112, [(1, 2, 2, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)]),      # six blocks per MCU, 8 x 7 MCUs
    "444": (120, 72, [(1, 1, 1, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)]),      # 15 x 9 MCUs
    "422": (128, 104, [(1, 2, 1, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)]),     # 8 x 13 MCUs
}


@functools.lru_cache(maxsize=None)
def jpeg_of(layout):
    import jpeg_writer as jw

    w, h, comps = LAYOUTS[layout]
    return jw.write_baseline(w, h, comps, np.random.default_rng(4100 + w + h), density=0.03)[0]   # (short blocks: lanes of a few hundred bits fall into step inside one subsequence)


def slice_record(layout, start, trunc):
    """what lep_jpeg_open_slice answers: (exit code, hand-offs of the plan, the .lep written around EMPTY coder streams -- its header
    holds every hand-off row's state, the reduced JPEG header, the prefix garbage and the trailing garbage)"""
    from lepton_amd import abi

    L = abi.lib()
    jpg = jpeg_of(layout)
    n = min(len(jpg), trunc) if trunc else len(jpg)
    h = C.c_void_p()
    rc = L.lep_jpeg_open_slice(jpg, n, start, C.byref(h))
    if rc:
        return rc, [], b""
    ho = (abi.Handoff * 16)()
    k = L.lep_jpeg_plan_handoffs(h, 0, ho, 16)
    assert k >= 1
    streams = (abi.Bytes * k)()
    out = abi.Bytes()
    assert L.lep_jpeg_write_lep(h, 0, streams, k, C.byref(out)) == 0
    lep = out.tobytes()
    L.lep_free(out.data)
    L.lep_jpeg_close(h)
    hand = [(ho[i].luma_y_start, ho[i].luma_y_end, ho[i].segment_size, ho[i].overhang_byte, ho[i].num_overhang_bits, tuple(ho[i].last_dc)[:3]) for i in range(k)]
    return 0, hand, lep


@functools.lru_cache(maxsize=None)
def row_bytes(layout):
    """the byte (hand-off position) of every MCU row start behind the first, from the slice parser's own answers: the first kept row of a
    slice grows with start_byte, and row r's record stands at the largest start_byte that still keeps it"""
    jpg = jpeg_of(layout)
    w, h, comps = LAYOUTS[layout]
    vmax = max(c[2] for c in comps)
    mcuv = (h + 8 * vmax - 1) // (8 * vmax)

    def first_row(s):
        rc, hand, _ = slice_record(layout, s, 0)
        return hand[0][0] // vmax if not rc else mcuv + 1

    out = []
    for r in range(1, mcuv):
        lo, hi = 0, len(jpg)            # first_row(lo) <= r < first_row(hi)
        while hi - lo > 1:
            m = (lo + hi) // 2
            if first_row(m) <= r:
                lo = m
            else:
                hi = m
        out.append(lo)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def positions(layout):
    """(start_byte, trunc, what) for the layout: every kind of position the slice code distinguishes"""
    n = len(jpeg_of(layout))
    rows = row_bytes(layout)
    assert len(rows) >= 4 and list(rows) == sorted(set(rows)), rows
    mid, last = rows[len(rows) // 2], rows[-1]
    return (
        (0, 0, "whole file"),
        (40, 0, "start inside the header"),
        (mid, 0, "start exactly on a record's byte"),
        (mid - 1, 0, "one byte in front of a record"),
        (mid + 1, 0, "one byte behind a record"),
        (rows[0] - 1, 0, "one byte in front of the second row"),
        (last + 2, 0, "start in the last MCU row"),
        (n - 1, 0, "start behind the last row"),
        (n + 10, 0, "start behind the file"),
        (rows[0] + 3, rows[-2] + 5, "trunc inside the scan, start in front of it"),
        (0, mid + 7, "whole from the start, trunc inside the scan"),
        (mid + 3, mid - 20, "trunc in front of start"),
        (mid, mid, "trunc equal to start"),
    )
