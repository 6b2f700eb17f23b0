"""lep_gpu_decode_rows_retire on the GPU: q30_256x256_4seg (two thread segments) in a session on frames filled with 0xA5 -- one band of one
MCU row, segment 1 retired, then on to the end.  Segment 0 must finish with the rows of the one-shot decode; segment 1 must answer
status -2 with its rows_done frozen, every row of it at or behind rows_done must still hold the fill, and `running` must count it out.
The refusals (no session, an index out of range), a finished segment that is retired and stays finished, and a session that never
retires, which must give the records tests/test_gpu_decode_rows.py expects."""
import ctypes as C

import numpy as np
import pytest

from lepton_amd import abi
from test_decode_rows_emulation import frame_of, segment_rows
from test_gpu_decode_rows import bands_of, case

pytestmark = pytest.mark.gpu

FILL = 0xA5
NAME = "q30_256x256_4seg"
LEP_ASSERTION_FAILURE = 1


def test_retired_segment_stands_still_and_its_neighbour_finishes(gpu_codec):
    L, h = abi.lib(), gpu_codec.handle
    f, final = case(NAME)
    d = f.desc
    assert len(f.segments) == 2
    session = gpu_codec.decode_rows([f], 1, fill=FILL)
    try:
        first = next(session)                       # one band of one MCU row
        assert [p.status for p in first] == [-1, -1]
        frozen = list(first[1].rows_done)
        assert all(frozen[c] > segment_rows(d, f.segments[1], c)[0] for c in range(d.ncomp)), "segment 1 has decoded its first MCU row"
        second = session.send([1])                  # retire segment 1, then the next band
        assert second[1].status == -2 and list(second[1].rows_done) == frozen and second[0].status == -1
        # `running` counts the retired segment out (a band made directly: the frames are not fetched for it)
        prog, running = (abi.DecodeProgress * 2)(), C.c_int(-1)
        assert L.lep_gpu_decode_rows_advance(h, 1, prog, C.byref(running)) == 0
        assert running.value == 1 and prog[1].status == -2 and list(prog[1].rows_done) == frozen
        # an index out of range is refused and changes nothing; retiring the retired segment again changes nothing
        assert L.lep_gpu_decode_rows_retire(h, (C.c_int32 * 1)(2), 1) == LEP_ASSERTION_FAILURE and "index" in gpu_codec.last_error()
        assert L.lep_gpu_decode_rows_retire(h, (C.c_int32 * 2)(0, -1), 2) == LEP_ASSERTION_FAILURE
        assert L.lep_gpu_decode_rows_retire(h, (C.c_int32 * 1)(1), 1) == 0
        last, advances = second, 3
        for progress in session:
            assert progress[1].status == -2 and list(progress[1].rows_done) == frozen
            assert (progress[1].fail_component, progress[1].fail_y, progress[1].fail_x) == (-1, -1, -1)
            last = progress
            advances += 1
    finally:
        session.close()
    assert last[0].status == 0 and advances == bands_of(f, f.segments[0], 1)   # the session ends with segment 0, not with segment 1's rows
    got = frame_of(d)
    for c in range(d.ncomp):
        lo, hi = segment_rows(d, f.segments[0], c)
        assert np.array_equal(got[c][lo:hi], final[c][lo:hi]), "segment 0 is not the one-shot decode's"
        lo, hi = segment_rows(d, f.segments[1], c)
        assert np.array_equal(got[c][lo:frozen[c]], final[c][lo:frozen[c]]), "a row of segment 1 below rows_done is not final"
        assert frozen[c] < hi and (got[c][frozen[c]:hi] == FILL).all(), "a row of segment 1 behind rows_done was touched"


def test_retire_without_a_session_is_refused(gpu_codec):
    L, h = abi.lib(), gpu_codec.handle
    assert L.lep_gpu_decode_rows_retire(h, (C.c_int32 * 1)(0), 1) == LEP_ASSERTION_FAILURE
    assert "lep_gpu_decode_rows_retire" in gpu_codec.last_error() and "no decode session" in gpu_codec.last_error()


def test_retiring_a_finished_segment_changes_nothing(gpu_codec):
    f, final = case("c420_odd_203x149")     # one segment
    session = gpu_codec.decode_rows([f], 0, fill=FILL)
    try:
        done = next(session)
        assert done[0].status == 0
        with pytest.raises(StopIteration):
            session.send([0])
    finally:
        session.close()
    got = frame_of(f.desc)
    assert all(np.array_equal(got[c], final[c]) for c in range(f.desc.ncomp))


def test_retire_before_the_first_band(gpu_codec):
    """a fresh segment that is retired is never begun: its rows hold the fill, its record says no row"""
    L, h = abi.lib(), gpu_codec.handle
    f, final = case(NAME)
    d = f.desc
    dev = (abi.ImageDesc * 1)(d)   # through the calls themselves: begin, retire 1, one advance to the end
    owned = []

    def dmalloc(n):
        p = C.c_void_p()
        assert L.lep_gpu_malloc(h, n, C.byref(p)) == 0
        owned.append(p)
        return p

    try:
        for c in range(d.ncomp):
            p = dmalloc(d.nblocks(c) * 128 + 256)
            assert L.lep_gpu_memset(h, p, FILL, d.nblocks(c) * 128) == 0
            dev[0].blocks[c] = p.value
        blob, offs = b"", [0]
        for st in f.streams:
            blob += st + bytes(-len(st) % 256)
            offs.append(len(blob))
        d_streams, d_lens = dmalloc(len(blob) + 256), dmalloc(8)
        lens = (C.c_uint32 * 2)(*[len(st) for st in f.streams])
        assert L.lep_gpu_memcpy_h2d(h, d_streams, blob, len(blob)) == 0 and L.lep_gpu_memcpy_h2d(h, d_lens, lens, 8) == 0
        segs = (abi.Segment * 2)(*[abi.Segment(0, s.luma_y_start, s.luma_y_end, s.is_last) for s in f.segments])
        assert L.lep_gpu_decode_rows_begin(h, dev, 1, segs, 2, d_streams, (C.c_uint64 * 3)(*offs), d_lens, None) == 0
        try:
            assert L.lep_gpu_decode_rows_retire(h, (C.c_int32 * 1)(1), 1) == 0
            prog, running = (abi.DecodeProgress * 2)(), C.c_int(-1)
            assert L.lep_gpu_decode_rows_advance(h, 0, prog, C.byref(running)) == 0
            assert running.value == 0 and prog[0].status == 0 and prog[1].status == -2 and list(prog[1].rows_done) == [0, 0, 0]
            for c in range(d.ncomp):
                assert L.lep_gpu_memcpy_d2h(h, d.blocks[c], dev[0].blocks[c], d.nblocks(c) * 128) == 0
        finally:
            assert L.lep_gpu_decode_rows_end(h) == 0
    finally:
        for p in owned:
            L.lep_gpu_free(h, p)
    got = frame_of(d)
    for c in range(d.ncomp):
        lo, hi = segment_rows(d, f.segments[0], c)
        assert np.array_equal(got[c][lo:hi], final[c][lo:hi])
        lo, hi = segment_rows(d, f.segments[1], c)
        assert (got[c][lo:hi] == FILL).all()


@pytest.mark.parametrize("band", [1, 3])
def test_a_session_that_never_retires_is_what_it_was(gpu_codec, band):
    f, final = case(NAME)
    history = [[], []]
    for progress in gpu_codec.decode_rows([f], band, fill=FILL):
        for k, p in enumerate(progress):
            history[k].append(p)
    want = [bands_of(f, s, band) for s in f.segments]
    assert all(len(hh) == max(want) for hh in history)
    for hh, n in zip(history, want):
        assert [p.status for p in hh] == [-1] * (n - 1) + [0] * (len(hh) - n + 1)
        assert all(p.fail_component == p.fail_y == p.fail_x == -1 for p in hh)
    got = frame_of(f.desc)
    assert all(np.array_equal(got[c], final[c]) for c in range(f.desc.ncomp))
