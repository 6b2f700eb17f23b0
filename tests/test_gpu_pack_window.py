"""lep_gpu_pack_window_device (lepton_amd/csrc/lep_pack.h) on the GPU: of every run only the bytes [skip, min(len, skip + take)) moved back
to back -- exact bytes, offsets and total against numpy, for 1, 65 and 1100 runs (a wavefront of the offsets kernel holds 64 x 16 = 1024
lengths: with 1100 a wave total goes through LDS), lengths 0..300 and a few of ~70 KB, the windows of the CPU test
(tests/test_pack_window_emulation.py: starts and ends at every offset mod 4, skip == length, skip > length, take 0, windows that end
behind the run -- the device's lengths are shorter than the window's end there).  A canary stands in front of the destination and behind
d_dst_off[n]; a total beyond the cap copies nothing and still reports the total; lep_gpu_pack_device on the same runs is unchanged."""
import ctypes as C

import numpy as np
import pytest

from lepton_amd.codec import _check
from test_gpu_pack import BEHIND, CANARY, FRONT, check, pack, source
from test_pack_window_emulation import windows_of

pytestmark = pytest.mark.gpu


def pack_window(codec, src, offs, lens, skips, takes, cap_short=0):
    """(destination buffer with its canaries, d_dst_off, the true total)"""
    L, h = codec._L, codec.handle
    n = len(lens)
    total = int(sum(window(k, s, t) for k, s, t in zip(lens, skips, takes)))
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
        sk = (C.c_uint32 * n)(*[int(s) for s in skips])
        tk = (C.c_uint32 * n)(*[int(t) for t in takes])
        _check(L.lep_gpu_pack_window_device(h, d_src, so, d_len, sk, tk, n, d_dst.value + FRONT, total - cap_short, d_off, None), "lep_gpu_pack_window_device")
        _check(L.lep_gpu_sync(h), "lep_gpu_sync")
        out = np.zeros(room, dtype=np.uint8)
        _check(L.lep_gpu_memcpy_d2h(h, out.ctypes.data, d_dst, room), "d2h")
        off = np.zeros(n + 1, dtype=np.uint64)
        _check(L.lep_gpu_memcpy_d2h(h, off.ctypes.data, d_off, 8 * (n + 1)), "d2h")
        return out, off, total
    finally:
        for p in owned:
            L.lep_gpu_free(h, p)


def window(length, skip, take):
    return 0 if length <= skip else min(length - skip, take)


def runs(n, seed):
    """n runs: lengths 0..300 and a few of ~70 KB, each with one of the CPU test's windows for its length, every window in turn"""
    rng = np.random.default_rng(seed)
    lens = [int(k) for k in rng.integers(0, 301, n)]
    for i in range(0, n, 97):
        lens[i] = 70000 + int(rng.integers(0, 9))
    lens[n // 2] = 0
    skips, takes = [], []
    for i, k in enumerate(lens):
        w = windows_of(k)
        s, t = w[(i * 7 + seed) % len(w)]
        skips.append(s)
        takes.append(t)
    return lens, skips, takes


def check_window(out, off, total, src, offs, lens, skips, takes):
    wl = [window(k, s, t) for k, s, t in zip(lens, skips, takes)]
    want = np.concatenate([src[o + s:o + s + w] for o, s, w in zip(offs, skips, wl)]) if total else np.zeros(0, dtype=np.uint8)
    assert off.tolist() == [0] + np.cumsum(np.asarray(wl, dtype=np.uint64)).tolist()
    assert (out[:FRONT] == CANARY).all(), "bytes in front of d_dst were written"
    assert (out[FRONT + total:] == CANARY).all(), "bytes behind d_dst_off[n] were written"
    assert np.array_equal(out[FRONT:FRONT + total], want)


@pytest.mark.parametrize("n", [1, 65, 1100])
def test_windows_are_packed_back_to_back(gpu_codec, n):
    for seed in (1, 2):
        lens, skips, takes = runs(n, seed)
        if n > 1:
            assert any(s == k for k, s in zip(lens, skips)) or any(s > k for k, s in zip(lens, skips))
            assert any(t == 0 for t in takes) and any(s < k < s + t for k, s, t in zip(lens, skips, takes))
        src, offs = source(lens, np.random.default_rng(n + seed))
        out, off, total = pack_window(gpu_codec, src, offs, lens, skips, takes)
        check_window(out, off, total, src, offs, lens, skips, takes)
        assert b"lep_pack_window" in gpu_codec._L.lep_gpu_last_kernel_name(gpu_codec.handle)
        # the unwindowed pack of the same runs is what it was
        out, off, total = pack(gpu_codec, src, offs, lens)
        check(out, off, total, src, offs, lens)


def test_every_window_of_the_cpu_test_on_one_length(gpu_codec):
    """one launch per length class: every window of a run of 0, 5, 64, 259 bytes, each run at the next source alignment"""
    lens, skips, takes = [], [], []
    for k in (0, 5, 64, 259):
        for s, t in windows_of(k):
            lens.append(k); skips.append(s); takes.append(t)
    rng = np.random.default_rng(11)
    offs, at = [], 0
    for i, k in enumerate(lens):
        at += 1 + i % 5
        offs.append(at)
        at += k
    src = rng.integers(0, 256, at + 64, dtype=np.uint8)
    out, off, total = pack_window(gpu_codec, src, offs, lens, skips, takes)
    check_window(out, off, total, src, offs, lens, skips, takes)


def test_a_capacity_one_byte_short_copies_nothing(gpu_codec):
    lens, skips, takes = runs(65, 3)
    src, offs = source(lens, np.random.default_rng(3))
    out, off, total = pack_window(gpu_codec, src, offs, lens, skips, takes, cap_short=1)
    assert total > 0 and int(off[-1]) == total, "d_dst_off[n] must hold the true total"
    assert (out == CANARY).all(), "something was copied although the total exceeds d_dst_cap"


def test_refusals(gpu_codec):
    L, h = gpu_codec._L, gpu_codec.handle
    one64, one32 = (C.c_uint64 * 1)(0), (C.c_uint32 * 1)(0)
    assert L.lep_gpu_pack_window_device(h, None, one64, None, one32, one32, 16385, None, 0, None, None) != 0
    assert b"lep_gpu_pack_window_device" in gpu_codec._L.lep_gpu_last_error(h)
