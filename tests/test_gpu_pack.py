"""lep_gpu_pack_device (lepton_amd/csrc/lep_pack.h) on the GPU: byte runs that lie apart in device memory, at odd offsets, moved back to
back; the prefix sum of their lengths; nothing written in front of the destination or behind the total; nothing at all when the total
exceeds the destination's capacity."""
import ctypes as C

import numpy as np
import pytest

from lepton_amd.codec import _check

pytestmark = pytest.mark.gpu

CANARY = 0xEE
FRONT = 67          # canary bytes in front of d_dst: the destination itself starts at an odd address
BEHIND = 4096


def pack(codec, src, offs, lens, cap_short=0):
    """runs (offs[i], lens[i]) of the host array `src` through the kernel: (destination buffer with its canaries, d_dst_off, total)"""
    L, h = codec._L, codec.handle
    n = len(lens)
    total = int(sum(lens))
    cap = total - cap_short
    owned = []

    def dmalloc(k):
        p = C.c_void_p()
        _check(L.lep_gpu_malloc(h, max(k, 16), C.byref(p)), "lep_gpu_malloc")
        owned.append(p)
        return p

    try:
        d_src = dmalloc(len(src))
        _check(L.lep_gpu_memcpy_h2d(h, d_src, src.ctypes.data, len(src)), "h2d")
        d_len = dmalloc(4 * n)
        hl = np.asarray(lens, dtype=np.uint32)
        _check(L.lep_gpu_memcpy_h2d(h, d_len, hl.ctypes.data, 4 * n), "h2d")
        room = FRONT + total + BEHIND
        d_dst = dmalloc(room)
        _check(L.lep_gpu_memset(h, d_dst, CANARY, room), "memset")
        d_off = dmalloc(8 * (n + 1))
        _check(L.lep_gpu_memset(h, d_off, 0xFF, 8 * (n + 1)), "memset")
        so = (C.c_uint64 * n)(*[int(o) for o in offs])
        _check(L.lep_gpu_pack_device(h, d_src, so, d_len, n, d_dst.value + FRONT, cap, d_off, None), "lep_gpu_pack_device")
        _check(L.lep_gpu_sync(h), "lep_gpu_sync")
        out = np.zeros(room, dtype=np.uint8)
        _check(L.lep_gpu_memcpy_d2h(h, out.ctypes.data, d_dst, room), "d2h")
        off = np.zeros(n + 1, dtype=np.uint64)
        _check(L.lep_gpu_memcpy_d2h(h, off.ctypes.data, d_off, 8 * (n + 1)), "d2h")
        return out, off, total
    finally:
        for p in owned:
            L.lep_gpu_free(h, p)


def source(lens, rng):
    """a source array with the runs at odd, ascending offsets with gaps between them"""
    offs, at = [], 1
    for k in lens:
        offs.append(at)
        at += k + 1 + int(rng.integers(0, 17))      # behind the run and a gap ...
        at |= 1                                      # ... at the next odd offset
    src = rng.integers(0, 256, at + 64, dtype=np.uint8)
    assert all(o % 2 == 1 for o in offs)
    return src, offs


def check(out, off, total, src, offs, lens):
    want = np.concatenate([src[o:o + k] for o, k in zip(offs, lens)]) if total else np.zeros(0, dtype=np.uint8)
    assert off.tolist() == [0] + np.cumsum(np.asarray(lens, dtype=np.uint64)).tolist()
    assert (out[:FRONT] == CANARY).all(), "bytes in front of d_dst were written"
    assert (out[FRONT + total:] == CANARY).all(), "bytes behind d_dst_off[n] were written"
    assert np.array_equal(out[FRONT:FRONT + total], want)


CASES = {
    "one_empty_run": [0],
    "one_byte": [1],
    "mixed": [(0, 1, 3, 15, 16, 17, 63, 64, 65, 4095, 4097)[i % 11] for i in range(65)],
    "one_long_run": [(1 << 20) + 3],
}


@pytest.mark.parametrize("name", list(CASES))
def test_runs_are_packed_back_to_back(gpu_codec, name):
    lens = CASES[name]
    rng = np.random.default_rng(len(lens) * 31 + lens[0])
    src, offs = source(lens, rng)
    out, off, total = pack(gpu_codec, src, offs, lens)
    check(out, off, total, src, offs, lens)


def test_every_alignment_of_source_and_destination(gpu_codec):
    """runs of 5 .. 12 bytes after each other: the running destination offset and the sources pass through every pair of alignments"""
    lens = [5 + (i * 7) % 8 for i in range(64)]
    rng = np.random.default_rng(7)
    offs, at = [], 0
    for i, k in enumerate(lens):
        at += 1 + i % 5
        offs.append(at)
        at += k
    src = rng.integers(0, 256, at + 64, dtype=np.uint8)
    out, off, total = pack(gpu_codec, src, offs, lens)
    check(out, off, total, src, offs, lens)


def test_a_capacity_one_byte_short_copies_nothing(gpu_codec):
    lens = CASES["mixed"]
    rng = np.random.default_rng(3)
    src, offs = source(lens, rng)
    out, off, total = pack(gpu_codec, src, offs, lens, cap_short=1)
    assert int(off[-1]) == total, "d_dst_off[n] must hold the true total"
    assert (out == CANARY).all(), "something was copied although the total exceeds d_dst_cap"
