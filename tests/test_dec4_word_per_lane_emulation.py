"""The v4 decoder's owner updates with one Branch word per lane (lep_dec4.h adapt_words / regroup, lep_wave.h wave_gather) and its refill
test once per group of bins (BoolDec4 / BoolDec4S ensure + get_raw), stepped on the CPU through tests/emu/dec4_update_emu.cc: the one-word
pass against bupd_t for every count pair, the lane gather against an index loop, whole segments, cut streams and the resumable form against
the oracle -- in both forms of the serial rounds (the shipped assignment and -DLEP_DEC4_SCALAR=13)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
from conftest import ROOT, golden
from lepton_amd import abi, corpus
from lepton_amd.codec import JpegImage

FILL = 0x5A
I32P, U32P = C.POINTER(C.c_int32), C.POINTER(C.c_uint32)


def _build(name, flags):
    src = os.path.join(ROOT, "tests", "emu", "dec4_update_emu.cc")
    so = os.path.join(ROOT, "tests", "emu", "libcore_emu_dec4upd%s.so" % name)
    tmp = "%s.%d" % (so, os.getpid())
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared"] + flags + ["-o", tmp, src])
    os.replace(tmp, so)
    L = C.CDLL(so)
    L.emu_dec4_bupd_t.restype = C.c_uint32
    L.emu_dec4_bupd_t.argtypes = [C.c_uint32, C.c_uint32]
    L.emu_decode_segment_v4_rows.argtypes = [C.POINTER(abi.ImageDesc), C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_uint32, C.c_int,
                                             C.POINTER(abi.DecodeProgress), C.c_int, C.POINTER(C.c_uint32)]
    return L


@pytest.fixture(scope="module", params=["shipped", "scalar13"])
def emu(request):
    L = _build("_" + request.param, [] if request.param == "shipped" else ["-DLEP_DEC4_SCALAR=13"])
    knobs = L.emu_dec4_knobs()
    assert knobs & 3 == 3, "the emulation was not built with both new forms on"
    assert knobs >> 8 == (2 if request.param == "shipped" else 13)
    return L


@pytest.fixture(scope="module")
def emu1():
    return _build("_shipped", [])


def arr(a, t):
    return np.ascontiguousarray(a, dtype=t)


def ptr(a, t):
    return a.ctypes.data_as(t)


# ---- the one-word pass against bupd_t ----------------------------------------------------------------------------------------------------
def test_one_word_pass_equals_bupd_t_for_every_count_pair(emu1):
    """every count pair 1..255 x 1..255 under BOTH observations with every lane used (trials 0 and 1: all 65025 pairs each, so every
    255-wrap, the halving path and the f = 1 / t = 1 special cases of either observation), then used and unused lanes mixed 64 at a time
    (trials 2 and 3): used lanes == bupd_t, unused lanes unchanged"""
    f, t = np.meshgrid(np.arange(1, 256, dtype=np.uint32), np.arange(1, 256, dtype=np.uint32), indexing="ij")
    rng = np.random.default_rng(16)
    probs = rng.integers(0, 256, f.size, dtype=np.uint32)
    words = (f.ravel() | (t.ravel() << 8) | (probs << 16)).astype(np.uint32)
    pad = (-words.size) % 64
    words = np.concatenate([words, words[:pad]])
    want = {obs: np.array([emu1.emu_dec4_bupd_t(int(w), obs) for w in words], dtype=np.uint32) for obs in (0, 1)}
    wraps = {0: 0, 1: 0}
    mixed_use, mixed_obs = arr(rng.integers(0, 2, words.size), np.int32), arr(rng.integers(0, 2, words.size), np.int32)
    for trial in range(4):
        use = np.ones(words.size, np.int32) if trial < 2 else mixed_use
        obs = np.full(words.size, trial, np.int32) if trial < 2 else (mixed_obs if trial == 2 else 1 - mixed_obs)
        got = words.copy()
        for o in range(0, words.size, 64):
            emu1.emu_dec4_adapt_words(ptr(got[o:o + 64], U32P), ptr(use[o:o + 64], I32P), ptr(obs[o:o + 64], I32P))
        expect = np.where(use == 1, np.where(obs == 1, want[1], want[0]), words)
        bad = np.flatnonzero(got != expect)
        assert bad.size == 0, (trial, hex(int(words[bad[0]])), int(use[bad[0]]), int(obs[bad[0]]), hex(int(got[bad[0]])), hex(int(expect[bad[0]])))
        if trial < 2:   # the pairs whose bumped count wraps: 255 per observation (+ the padding's repeats), all of them run
            wrapped = ((words & 255) == 255) if trial == 0 else (((words >> 8) & 255) == 255)
            wraps[trial] = int(wrapped[:f.size].sum())
            assert (got[:f.size][wrapped[:f.size]] != words[:f.size][wrapped[:f.size]] + (1 if trial == 0 else 256)).all()   # not the plain bump
    assert wraps == {0: 255, 1: 255}
    one = {(1, 255, 1), (255, 1, 0)}   # the saturating special cases of bupd_t: the other count is 1
    for fv, tv, o in one:
        w = np.array([fv | (tv << 8) | (77 << 16)] * 64, dtype=np.uint32)
        emu1.emu_dec4_adapt_words(ptr(w, U32P), ptr(np.ones(64, np.int32), I32P), ptr(np.full(64, o, np.int32), I32P))
        assert (w == ((fv | (tv << 8)) | ((0 if o else 255) << 16))).all(), (fv, tv, o, hex(int(w[0])))


# ---- wave_gather -------------------------------------------------------------------------------------------------------------------------
def _combo_base(j):
    return [0, 7, 13, 18, 22, 25, 27][j]


def _lane_maps():
    """(name, src[64], slot[64]) of identity, reversal and the rounds' lane maps for sample outcomes of their serial code"""
    rng = np.random.default_rng(3)
    lanes = np.arange(64)
    maps = [("identity", lanes.copy(), lanes & 3), ("reversal", 63 - lanes, lanes & 3)]
    for nz in (0, 1, 37, 49, 63):   # round_nz: lane t < 6 = tree level 5 - t
        src, slot = lanes.copy() * 0, lanes * 0
        for t in range(6):
            prefix = nz >> (5 - t + 1)
            src[t] = [0, 1, 2, 3, 5, 9][t] + (prefix >> 2)
            slot[t] = prefix & 3
        maps.append(("nz_%d" % nz, src, slot))
    for k in range(3):              # round_77, exponent and residual words: lane = pi + 16 * slot, source = pi + 16 * candidate in force at pi
        cand = np.sort(rng.integers(0, 4, 16))
        maps.append(("77_%d" % k, (lanes & 15) + 16 * cand[lanes & 15], lanes >> 4))
    for k in range(3):              # round_edges: lanes 4 * (e * 7 + j) + slot from combo lane e * 28 + combo_base(j) + left - 1; 56..61 themselves
        src, slot = lanes.copy(), lanes & 3
        for e in range(2):
            left = int(rng.integers(1, 8))
            for j in range(7):
                if 1 <= left <= 7 - j:
                    src[4 * (e * 7 + j):4 * (e * 7 + j) + 4] = e * 28 + _combo_base(j) + left - 1
                    left -= int(rng.integers(0, 2))
        slot[56:62] = rng.integers(0, 4, 6)
        maps.append(("edges_%d" % k, src, slot))
    src, slot = lanes.copy(), lanes * 0   # round_dc: lanes 0..10 exponent word l of group l / 4, lanes 11..20 the residual Branch of lane l - 8
    src[:11], slot[:11] = lanes[:11] >> 2, lanes[:11] & 3
    src[11:21] = lanes[11:21] - 8
    maps.append(("dc", src, slot))
    return maps


@pytest.mark.parametrize("case", _lane_maps(), ids=lambda c: c[0])
def test_wave_gather_equals_an_index_loop(emu1, case):
    _, src, slot = case
    rng = np.random.default_rng(5)
    v = arr(rng.integers(0, 1 << 32, 64, dtype=np.uint64), np.uint32)
    s32, k32 = arr(src, np.int32), arr(slot, np.int32)
    out = np.zeros(64, np.uint32)
    emu1.emu_wave_gather(ptr(v, U32P), ptr(s32, I32P), ptr(out, U32P))
    assert np.array_equal(out, np.array([v[src[l]] for l in range(64)], dtype=np.uint32))
    groups = arr(rng.integers(0, 1 << 32, 256, dtype=np.uint64), np.uint32)
    emu1.emu_dec4_regroup(ptr(groups, U32P), ptr(s32, I32P), ptr(k32, I32P), ptr(out, U32P))
    assert np.array_equal(out, np.array([groups[4 * src[l] + slot[l]] for l in range(64)], dtype=np.uint32))


# ---- whole segments against the oracle ---------------------------------------------------------------------------------------------------
def _set_coefficients(img, fn):
    d = img.desc
    for c in range(d.ncomp):
        n = d.nblocks(c) * 64
        a = np.frombuffer((C.c_int16 * n).from_address(d.blocks[c]), dtype=np.int16)
        a[:] = fn(c, n)
    return img


def _large(c, n):
    rng = np.random.default_rng(5 + c)
    vals = rng.integers(-255, 256, n)
    vals[rng.random(n) < 0.1] = 0
    vals = vals.reshape(-1, 64)
    vals[:, 49] = 0
    return vals.ravel()


def _large_dc(c, n):
    """DC coefficients all over their range (deltas of up to 11 bits: every DC exponent word and all ten residual Branches), few ACs"""
    rng = np.random.default_rng(21 + c)
    vals = rng.integers(-2, 3, n).reshape(-1, 64)
    vals[rng.random(vals.shape) < 0.7] = 0
    vals[:, 49] = rng.integers(-1000, 1001, vals.shape[0])
    vals[::5, 49] = rng.integers(-3, 4, len(vals[::5]))   # and small deltas between them
    return vals.ravel()


def _interior_full(c, n):
    rng = np.random.default_rng(9 + c)
    vals = rng.integers(1, 40, n) * rng.choice([-1, 1], n)
    vals = vals.reshape(-1, 64)
    vals[:, 49:] = rng.integers(-3, 4, (vals.shape[0], 15))   # aligned order: 0..48 interior, 49 DC, 50..63 edges
    return vals.ravel()


def _images():
    out = {}
    for name in ("one_block_8x8", "one_col_8x64", "c420_odd_203x149", "gray_120x88"):
        out[name] = lambda name=name: JpegImage(golden(name)[0])
    out["large_64x48_q100"] = lambda: _set_coefficients(JpegImage(corpus.synth_jpeg(64, 48, 11, quality=100)), _large)
    out["large_dc_64x48"] = lambda: _set_coefficients(JpegImage(corpus.synth_jpeg(64, 48, 11, quality=100)), _large_dc)
    out["interior_full_64x48"] = lambda: _set_coefficients(JpegImage(corpus.synth_jpeg(64, 48, 11, quality=100)), _interior_full)
    out["all_zero_64x48"] = lambda: _set_coefficients(JpegImage(corpus.synth_jpeg(64, 48, 11)), lambda c, n: 0)
    return out


IMAGES = _images()
CASES = {}


def case(name):
    """once per image: (image, segments, oracle streams, oracle bins, frame bytes per component)"""
    if name not in CASES:
        img = IMAGES[name]()
        segs = img.plan()
        streams, bins = ob.oracle_encode(img.desc, segs)
        frame = [C.string_at(img.desc.blocks[c], img.desc.nblocks(c) * 128) for c in range(img.desc.ncomp)]
        CASES[name] = (img, segs, streams, bins, frame)
    return CASES[name]


def fill_frame(d):
    for c in range(d.ncomp):
        C.memset(d.blocks[c], FILL, d.nblocks(c) * 128)


def frame_of(d):
    return [C.string_at(d.blocks[c], d.nblocks(c) * 128) for c in range(d.ncomp)]


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_segments_equal_the_oracle(emu, name):
    img, segs, streams, bins, frame = case(name)
    d = img.desc
    fill_frame(d)
    total = 0
    for s, w in zip(segs, streams):
        nb = C.c_uint32(0)
        assert emu.emu_decode_segment_v4(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, w, len(w), C.byref(nb)) == 0
        total += nb.value
    assert total == bins
    for c in range(d.ncomp):
        n = d.coded_blocks[c] * 128
        assert C.string_at(d.blocks[c], n) == frame[c][:n]


@pytest.mark.parametrize("name", ["c420_odd_203x149", "large_64x48_q100", "large_dc_64x48", "one_block_8x8"])
def test_bands_of_one_mcu_row_give_the_one_shot_frame(emu, name):
    img, segs, streams, bins, frame = case(name)
    d = img.desc
    fill_frame(d)
    total = 0
    for s, w in zip(segs, streams):
        cap = d.mcu_rows + 2
        prog = (abi.DecodeProgress * cap)()
        nb = C.c_uint32(0)
        n = emu.emu_decode_segment_v4_rows(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, w, len(w), 1, prog, cap, C.byref(nb))
        assert n >= 1 and prog[n - 1].status == 0, (n, prog[max(n, 1) - 1].status)
        total += nb.value
    assert total == bins
    for c in range(d.ncomp):
        n = d.coded_blocks[c] * 128
        assert C.string_at(d.blocks[c], n) == frame[c][:n]


# ---- streams cut short -------------------------------------------------------------------------------------------------------------------
def cut_case():
    if "cut" not in CASES:
        img = JpegImage(corpus.synth_jpeg(203, 149, 7))
        segs = img.plan()
        streams, _ = ob.oracle_encode(img.desc, segs)
        assert len(segs) == 1
        CASES["cut"] = (img, segs[0], streams[0])
    return CASES["cut"]


def oracle_on(d, s, data):
    fill_frame(d)
    im = ob.to_lor(d)
    buf = C.create_string_buffer(data, len(data)) if data else C.create_string_buffer(1)
    rc = ob.oracle().lor_decode_segment(C.byref(im), s.luma_y_start, s.luma_y_end, s.is_last, buf, len(data), None)
    return rc, frame_of(d)


def same_frame_up_to_the_refused_block(d, rc, got, want):
    """exit code 0: the frames are equal.  Otherwise they are equal but for the ONE block the decoder refused, which it does not store
    (lep_dec4.h run: "that block is not stored, everything in front of it is") and the oracle has written into"""
    differ = []
    for c in range(d.ncomp):
        g = np.frombuffer(got[c], dtype=np.uint8).reshape(-1, 128)
        w = np.frombuffer(want[c], dtype=np.uint8).reshape(-1, 128)
        differ += [(c, int(b), bool((g[b] == FILL).all())) for b in np.flatnonzero((g != w).any(axis=1))]
    if rc == 0:
        assert differ == []
        return
    assert len(differ) <= 1 and all(untouched for _, _, untouched in differ), differ[:4]
    for c, b, _ in differ:   # ... and it is the first block not stored: nothing of its component behind it is touched, in either frame
        for f in (got, want):
            assert (np.frombuffer(f[c], dtype=np.uint8).reshape(-1, 128)[b + 1:] == FILL).all()
        assert (np.frombuffer(got[c], dtype=np.uint8).reshape(-1, 128)[b:] == FILL).all()


def cut_lengths(n):
    return [0, 1, 2, 3, 5, 8, 13, 64, 200, n // 2, n - 1]


@pytest.mark.parametrize("k", range(11))
def test_cut_streams_end_as_the_oracle_s_do(emu, k):
    img, s, stream = cut_case()
    d = img.desc
    data = stream[:cut_lengths(len(stream))[k]]
    want_rc, want_frame = oracle_on(d, s, data)
    fill_frame(d)
    rc = emu.emu_decode_segment_v4(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, data, len(data), None)
    assert rc == want_rc
    one_shot = frame_of(d)
    same_frame_up_to_the_refused_block(d, rc, one_shot, want_frame)
    # the resumable form names the block it refused: the differing block is that one, the first unstored block in schedule order
    from test_decode_rows_emulation import check_failing_block, frame_of as rows_frame_of
    fill_frame(d)
    cap = d.mcu_rows + 2
    prog = (abi.DecodeProgress * cap)()
    n = emu.emu_decode_segment_v4_rows(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, data, len(data), 0, prog, cap, None)
    assert n >= 1
    assert frame_of(d) == one_shot
    got_rows = rows_frame_of(d)
    C.memmove(d.blocks[0], want_frame[0], len(want_frame[0]))   # the oracle's frame once more, in that helper's layout
    for c in range(1, d.ncomp):
        C.memmove(d.blocks[c], want_frame[c], len(want_frame[c]))
    check_failing_block(d, s, want_rc, rows_frame_of(d), prog[n - 1], got_rows)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_stream_that_starts_inside_a_dword(emu, shift):
    img, segs, streams, bins, frame = case("c420_odd_203x149")
    d = img.desc
    fill_frame(d)
    for s, w in zip(segs, streams):
        arena = C.create_string_buffer(b"\xff" * 8 + b"\xa5" * shift + w + b"\x5a" * 9)   # poison either side
        base = C.addressof(arena)
        base += (-base) % 4 + 4
        C.memmove(base + shift, w, len(w))
        C.memset(base, 0xA5, shift)
        C.memset(base + shift + len(w), 0x5A, 8)
        assert emu.emu_decode_segment_v4(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, C.c_void_p(base + shift), len(w), None) == 0
    for c in range(d.ncomp):
        n = d.coded_blocks[c] * 128
        assert C.string_at(d.blocks[c], n) == frame[c][:n]
