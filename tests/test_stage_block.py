"""lepbuf::Block (lepton_amd/csrc/lep_block.h) -- the descriptor block that every launch path of lep_gpu.hip stages through the pinned
ring: a Layout that remembers where its parts come from -- through tests/emu/stage_block_probe.cc, on the part sequences of the workspaces
that are staged.  The expected offsets and images below are worked out here, with Python's integers and numpy slices, none is taken from
the header:
  a part lies at the next multiple of its alignment behind the part before it;
  upload_bytes is the end of the last part that has a source and an element (0 where there is none);
  the image of [0, upload_bytes) has every sourced part at its offset and zero bytes everywhere else."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "emu", "stage_block_probe.cc")
COUNTS, ALIGNS = (0, 1, 3, 1000), (4, 16, 256)
# workspace -> its parts in order: (element bytes, has a source); the sizes are those of the types in the comments, held to them by the
# static assertions above stage() in lep_gpu.hip (LEP_STAGED): a type that changes size stops the build and names this table
WORKSPACES = {
    "W_META": [(2208, 1), (32, 1), (8, 1), (4, 0)],                     # ImageDev | SegDev | ns offsets | bins
    "W_HUFF": [(4272, 1), (40, 1)],                                     # HuffImage | HuffSegment
    "W_HUFFENC": [(40, 1), (8, 1), (4, 0), (1, 0)],                     # SimtEncSeg | SimtEncWave | unit words | bit buffers
    "W_PACK": [(8, 1)],                                                 # source offsets
    "W_PACK window": [(8, 1), (4, 1), (4, 1), (4, 0)],                  # source offsets | skip | take | clipped lengths
    "W_SAMPLES": [(176, 1), (4, 1)],                                    # PlaneRec | first
    "W_HUFFPROG": [(168, 1), (4184, 1)],                                # ProgImage | ProgScan
    "W_HUFFSEQ": [(4, 1), (4, 1), (4, 0), (16, 0)],                     # which | caps | byte counts | end states
    "W_HUFFPROGSIMT": [(48, 1), (8, 1), (24, 1), (4, 0), (1, 0)],       # ProgSimtScan | ProgSimtWave | ProgSimtRegion | unit words | bit buffers
    "W_HUFFPROGDEC pipelined": [(5696, 1), (16, 1), (4, 0)],            # ProgDecScan | ProgDeps | progress words
    "W_HUFFPROGDEC by level": [(5696, 1), (16, 0), (4, 0)],             # ... the dependencies without a source
    "W_HUFFPROGRST": [(5696, 1), (5696, 1), (16, 1), (24, 0)],          # ProgDecScan (plain) | ProgDecScan | ProgRstScan | ProgRstOut
    "W_HUFFDEC": [(5552, 1)],                                           # HuffDecImage
    "W_HUFFPAR": [(36, 1), (8, 1), (20, 0), (20, 0), (12, 0), (32, 0)],  # SimtImage | SimtWave | SimtSub x 2 | SimtPlace | SimtSlots
}


def blocks():
    """(workspace, [(element bytes, count, alignment, sourced)]): per workspace and alignment every count in every part at once, the four
    counts in turn from every starting point, and four seeded draws"""
    rng = np.random.default_rng(26)
    out = []
    for name, parts in WORKSPACES.items():
        for a in ALIGNS:
            picks = [[n] * len(parts) for n in COUNTS] + [[COUNTS[(i + r) % 4] for i in range(len(parts))] for r in range(4)]
            picks += [[COUNTS[int(k)] for k in rng.integers(0, 4, len(parts))] for _ in range(4)]
            for counts in picks:
                out.append((name, [(e, n, a, s) for (e, s), n in zip(parts, counts)]))
    # a sourceless part IN FRONT of a sourced one is written as zero bytes; parts with alignments of their own
    out.append(("mixed", [(4, 3, 4, 1), (16, 3, 16, 0), (8, 1, 256, 1), (1, 1000, 4, 0)]))
    out.append(("mixed", [(12, 3, 4, 0), (4, 1, 16, 1)]))
    return out


@pytest.fixture(scope="module")
def probe():
    so = os.path.join(ROOT, "tests", "emu", "libstage_block_probe.so")
    tmp = "%s.%d" % (so, os.getpid())
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-o", tmp, SRC])
    os.replace(tmp, so)
    lib = C.CDLL(so)
    P = C.POINTER
    lib.emu_stage_block.argtypes = [P(C.c_uint32), P(C.c_uint64), P(C.c_uint32), P(C.c_int32), C.c_int, C.c_void_p, P(C.c_uint64), P(C.c_uint64), P(C.c_uint64), C.c_void_p]
    return lib


def expected(parts, src):
    """(offsets, bytes, upload_bytes, image) by the rules in the module's docstring"""
    offs, end, up, at, placed = [], 0, 0, 0, []
    for e, n, a, s in parts:
        off = -(-end // a) * a
        offs.append(off)
        end = off + n * e
        if s:
            if n:
                placed.append((off, at, n * e))
                up = end
            at += n * e
    image = np.zeros(up, dtype=np.uint8)
    for off, frm, nbytes in placed:
        image[off:off + nbytes] = src[frm:frm + nbytes]
    return offs, end, up, image


def run(probe, parts, src, guard=64):
    n = len(parts)
    arr = lambda t, k: (t * n)(*[p[k] for p in parts])
    ob, ol, totals = (C.c_uint64 * n)(), (C.c_uint64 * n)(), (C.c_uint64 * 5)()
    args = (arr(C.c_uint32, 0), arr(C.c_uint64, 1), arr(C.c_uint32, 2), arr(C.c_int32, 3), n, src.ctypes.data, ob, ol, totals)
    assert probe.emu_stage_block(*args, None) == 0
    image = np.full(int(totals[2]) + guard, 0xEE, dtype=np.uint8)
    assert probe.emu_stage_block(*args, image.ctypes.data) == 0
    return list(ob), list(ol), list(totals), image


def test_offsets_upload_bytes_and_image_of_every_workspace(probe):
    src = np.random.default_rng(1).integers(1, 256, 3 * 1000 * 5696, dtype=np.uint8)      # (never zero: a gap shows)
    seen_empty = 0
    for name, parts in blocks():
        ob, ol, (b_bytes, b_padded, up, l_bytes, l_padded), image = run(probe, parts, src)
        offs, end, want_up, want = expected(parts, src)
        assert ob == offs and ol == offs, (name, parts)
        assert b_bytes == l_bytes == end and b_padded == l_padded == -(-end // 256) * 256, (name, parts)
        assert up == want_up, (name, parts)
        assert np.array_equal(image[:up], want), (name, parts, "the image is not the parts copied one by one into a zeroed buffer")
        assert (image[up:] == 0xEE).all(), (name, parts, "pack() wrote behind upload_bytes")
        seen_empty += up == 0
    assert seen_empty >= 3 * len(WORKSPACES)        # every workspace with all its parts empty, at every alignment


def test_a_block_whose_sourced_parts_are_all_empty_uploads_nothing(probe):
    src = np.zeros(16, dtype=np.uint8)
    for parts in ([(8, 0, 256, 1), (4, 0, 256, 1), (4, 1000, 256, 0)], [(4, 1000, 4, 0), (8, 0, 16, 1)], [(5696, 0, 256, 1)], [(4, 3, 4, 0)]):
        ob, ol, totals, image = run(probe, parts, src)
        assert ob == ol == expected(parts, src)[0]
        assert totals[2] == 0 and (image == 0xEE).all(), parts


def test_an_element_size_the_probe_does_not_know_is_refused(probe):
    assert probe.emu_stage_block((C.c_uint32 * 1)(7), (C.c_uint64 * 1)(1), (C.c_uint32 * 1)(4), (C.c_int32 * 1)(0), 1, None, (C.c_uint64 * 1)(), (C.c_uint64 * 1)(), (C.c_uint64 * 5)(), None) == -1


def test_the_same_blocks_as_a_program_of_its_own_under_sanitizers(tmp_path):
    exe = str(tmp_path / "stage_block")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DSTAGE_BLOCK_MAIN", "-o", exe, SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)      # (no fallback: a compiler without the sanitizers' runtimes fails this test)
    assert r.returncode == 0, r.stderr[-3000:]
    cases = blocks()
    text = "".join("%d %s\n" % (len(parts), " ".join("%d %d %d %d" % p for p in parts)) for _, parts in cases)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout == "ok %d\n" % len(cases) and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout, r.stderr[-3000:])
