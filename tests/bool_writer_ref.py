"""A plain serial VP8 bool writer, the reference of the tests that run the split-phase encoder's writer kernels on raw bin lists
(tests/test_bool_writer_ref.py on the CPU, tests/test_gpu_enc5_writer_lists.py on the MI355X), and the seeded bin lists both see.

The writer is the reference's (boolwriter.hh:48-118 put, boolwriter.cc:17-35 finish) stated bin by bin: the start marker, the bins, 32
stop bins, then the end rule -- a stream whose last byte is 110xxxxx gets a zero byte appended.  It writes into a buffer without end;
what a writer with `cap` bytes of room does follows from the length L0 before the end rule: it overflows exactly when L0 >= cap, and
otherwise its bytes and length are this one's.

A bin list is a numpy uint16 array of probability | bit << 8 (the probability, 0..255, is that of a 0)."""
import numpy as np

WARM = 16384                       # lep_enc5.h kWarm5: bins a chunk's range run warms up over
STITCHED_K = (2, 4, 16, 64)        # chunks per segment of the stitched writer
PART_CUTS = ((8, 1), (8, 4), (3, 4), (2, 32))   # (parts, chunks per part) of the writer in part chunks
LANE_PARTS = (1, 3, 8)             # parts of the lane-per-segment writer
MAX_PARTS = 8

RANDOM = ("uniform", "low_mostly_1", "low_always_1", "high_mostly_0", "extremes", "drawn")
CONSTANT = {"const_0_255": (0, 255), "const_0_254": (0, 254), "const_1_1": (1, 1), "const_1_128": (1, 128), "const_0_128": (0, 128)}
FAMILIES = RANDOM + tuple(CONSTANT)
# 1 .. 129: lists shorter than the chunks are many, ends inside and on the edges of a 32-bin sector and of the 128 bins a list has room to;
# WARM - 1 .. WARM + 1: the warm-up reaches the stream's start or not; 2 * WARM - 2, 2 * WARM, 2 * WARM + 2: the chunk in the middle
# -- chunk K / 2 of every even K starts at bin n // 2 -- begins on bin WARM - 1, WARM, WARM + 1; 40,000 and 70,000: several chunks
# beyond the warm-up
LENGTHS = (1, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, WARM - 1, WARM, WARM + 1, 2 * WARM - 2, 2 * WARM, 2 * WARM + 2, 40000, 70000)
CAP_LENGTHS = (1, 5, 33, 129, WARM + 1, 2 * WARM + 2)   # the lists that are also written into reservations around their length
ROOMY = 1 << 17                    # no list here makes a stream this long (70,000 bins of at most 7 bits a bin are 61 KB)


def bool_write(bins):
    """(stream, L0): the bytes the serial writer makes of the list, end rule applied, and its length before the end rule"""
    a = np.asarray(bins, dtype=np.uint16)
    probs = [128] + (a & 255).tolist() + [128] * 32
    bits = [0] + ((a >> 8) & 1).tolist() + [0] * 32
    out = bytearray()
    low, rng, count = 0, 255, -24
    for bit, prob in zip(bits, probs):
        split = 1 + (((rng - 1) * prob) >> 8)
        if bit:
            low += split
            rng -= split
        else:
            rng = split
        shift = 8 - rng.bit_length()          # normalise: the range back into 128..255
        rng <<= shift
        count += shift
        if count >= 0:                         # a whole byte has left the 24 bits the recurrence works on
            offset = shift - count
            if (low << (offset - 1)) & 0x80000000:   # a carry: back through the 0xFF bytes
                x = len(out) - 1
                while x >= 0 and out[x] == 0xFF:
                    out[x] = 0
                    x -= 1
                if x >= 0:
                    out[x] += 1
            out.append((low >> (24 - offset)) & 255)
            low = (low << offset) & 0xFFFFFF
            shift = count
            count -= 8
        low = (low << shift) & 0xFFFFFFFF
    l0 = len(out)
    if l0 and (out[-1] & 0xE0) == 0xC0:
        out.append(0)
    return bytes(out), l0


def expect(stream, l0, cap):
    """what a writer with `cap` bytes of room must report: (overflow, bytes) -- the bytes are None where it overflows"""
    return (True, None) if l0 >= cap else (False, stream)


def bin_list(family, n, seed):
    rng = np.random.default_rng(seed)
    if family in CONSTANT:
        bit, prob = CONSTANT[family]
        return np.full(n, prob | bit << 8, dtype=np.uint16)
    if family == "uniform":
        prob, bit = rng.integers(0, 256, n), rng.integers(0, 2, n)
    elif family == "low_mostly_1":
        prob, bit = rng.integers(1, 4, n), (rng.integers(0, 8, n) != 0)
    elif family == "low_always_1":
        prob, bit = rng.integers(1, 4, n), np.ones(n, dtype=np.int64)
    elif family == "high_mostly_0":
        prob, bit = rng.integers(250, 256, n), (rng.integers(0, 8, n) == 0)
    elif family == "extremes":
        prob, bit = np.where(rng.integers(0, 2, n) == 1, 255, 1), rng.integers(0, 2, n)
    elif family == "drawn":
        prob = rng.integers(0, 256, n)
        bit = rng.integers(0, 256, n) >= prob
    else:
        raise ValueError(family)
    return (prob.astype(np.uint16) | (bit.astype(np.uint16) << 8)).astype(np.uint16)


_LISTS = {}


def lists():
    """once: [(family, bins)] -- every family at every length, 2.8 million bins in all"""
    if "all" not in _LISTS:
        _LISTS["all"] = [(f, bin_list(f, n, 1000 * i + j)) for i, f in enumerate(FAMILIES) for j, n in enumerate(LENGTHS)]
    return _LISTS["all"]


def references():
    """once: [(stream, L0)] of lists()"""
    if "ref" not in _LISTS:
        _LISTS["ref"] = [bool_write(b) for _, b in lists()]
    return _LISTS["ref"]


def cap_cases():
    """[(index into lists(), cap)]: the lists of CAP_LENGTHS of every family at L0 - 1, L0, L0 + 1, L0 + 2 and 1 byte of room"""
    out = []
    for i, ((_, b), (_, l0)) in enumerate(zip(lists(), references())):
        if len(b) in CAP_LENGTHS:
            out += [(i, max(l0 - 1, 0)), (i, l0), (i, l0 + 1), (i, l0 + 2), (i, 1)]
    return out


def part_bounds(n, parts, seed):
    """first bins of `parts` parts of a list of n bins as tests/emu/enc5_part_chunks_emu.cc check_lists draws them: sorted random places;
    every third draw some neighbours made equal (empty parts), every fifth the bounds crowded into a stretch of 40 bins (parts of a few bins)"""
    rng = np.random.default_rng(seed)
    span = min(n, 40) if seed % 5 == 0 else n
    start = int(rng.integers(0, n - span + 1))
    b = [0] + sorted(start + int(x) for x in rng.integers(0, span + 1, parts - 1))
    if seed % 3 == 0:
        for p in range(parts - 1, 0, -1):
            if rng.integers(0, 2):
                b[p] = b[p + 1] if p + 1 < parts else n
    return b


REC_WORDS = 16                      # lep_enc5.h WChunk5 as uint32: the fields below, then 7 unused
Q_GUESS, Q_END, SHIFTS, Q_START, T_START, KEEP, KEEP_BITS, CARRY, POS_END = range(9)


def chunk_counts(recs):
    """what one list's records (chunks x REC_WORDS, uint32) say the run exercised: (chunks behind the first whose guessed start range
    was wrong -- the link pass ran their range again --, chunks behind the first that start before the stream's first byte, chunks
    with a carry that left their own stretch)"""
    r = np.asarray(recs, dtype=np.uint32).reshape(-1, REC_WORDS)
    return (int((r[1:, Q_GUESS] != r[1:, Q_START]).sum()), int((r[1:, T_START] < 24).sum()), int((r[:, CARRY] != 0).sum()))


def say_counts(wrong, early, carries):
    """one line on {family: [(list length, wrong guesses)]} and the two other counts"""
    long_ = {f: [w for n, w in v if n > 2 * WARM] for f, v in wrong.items() if any(w for _, w in v)}
    short = sum(w for v in wrong.values() for n, w in v if n <= 2 * WARM)
    return "wrong guesses in the lists of over %d bins %s, in shorter lists %d; chunks with t_start < 24: %d; with a carry out: %d" % (2 * WARM, long_, short, early, carries)
