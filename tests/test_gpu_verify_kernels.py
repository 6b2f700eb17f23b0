"""The three kernels of the round-trip check on the MI355X, on buffers the test gives (lep_batch_debug_compare, lep_batch_debug_scan_check:
the launchers launch_compress_chunk uses, so the grid and the arguments are the product's): lep_compare_kernel, lep_scan_check_kernel and
lep_scan_check_bytes_kernel against tests/verify_ref.py.  Every case says itself whether the item differs, verify_ref must agree, and the
flag words after the launch must equal verify_ref's: the flag array is longer than the launch needs and pre-filled, so a word the launch
must not touch, or a bit that was set before, shows when it changes (atomicOr, not a store)."""
import numpy as np
import pytest

import verify_ref as vr

pytestmark = pytest.mark.gpu

GRID_LANES = 256 * 256          # lep_compare_kernel's grid: 256 workgroups of 256 lanes, 16 bytes per lane and pass
COMPARE_FILL = 0x5A5A5A5A       # bit 0, the compare kernel's, is clear
SCAN_FILL = 0xA5A5A5A5          # bit 1, the scan checks', is clear


def flipped(buf, byte, bit):
    out = buf.copy()
    out[byte] ^= np.uint8(1 << bit)
    return out


@pytest.mark.parametrize("units", [0, 1, 255, 256, GRID_LANES - 1, GRID_LANES, GRID_LANES + 1, 2 * GRID_LANES + 1])
def test_compare_kernel(gpu_codec, units):
    """sizes in 16-byte units around the grid's 65,536 lanes: one less, one more, and a third grid-stride pass"""
    rng = np.random.default_rng(units)
    nbytes = units * 16
    a = rng.integers(0, 256, nbytes + 16, dtype=np.uint8)      # one unit more than is compared
    flags = np.full(8, COMPARE_FILL, dtype=np.uint32)
    cases = [("equal", a, False), ("behind the compared length", flipped(a, nbytes + int(rng.integers(0, 16)), 3), False)]
    if units:
        cases += [("first unit", flipped(a, int(rng.integers(0, 16)), 0), True),
                  ("last unit", flipped(a, nbytes - 16 + int(rng.integers(0, 16)), 7), True),
                  ("last byte", flipped(a, nbytes - 1, 7), True)]
        mid = units // 2
        for dword in range(4):
            cases.append(("dword %d of unit %d" % (dword, mid), flipped(a, mid * 16 + dword * 4 + int(rng.integers(0, 4)), int(rng.integers(0, 8))), True))
    if units > GRID_LANES:
        cases.append(("unit 65,536: the second pass", flipped(a, GRID_LANES * 16 + 5, 2), True))
    if units > 2 * GRID_LANES:
        cases.append(("unit 131,072: the third pass", flipped(a, 2 * GRID_LANES * 16 + 12, 6), True))
    for k, (what, b, differs) in enumerate(cases):
        word, value = 1 + k % 6, (1, 1, 0x20)[k % 3]
        want = vr.compare_flags(a, b, nbytes, flags, word, value)
        assert bool(want[word] != flags[word]) == differs, what
        for x, y in ((a, b), (b, a)):
            got = gpu_codec.debug_compare(x, y, nbytes, flags, word, value)
            assert np.array_equal(got, want), (units, what, [hex(v) for v in got])
    # a flag word that already holds the bit, and one that holds every other bit: both keep what they had
    for fill in (0xFFFFFFFF, 0xFFFFFFFE, 1):
        f2 = np.full(4, fill, dtype=np.uint32)
        for what, b, _ in cases[:5]:
            assert np.array_equal(gpu_codec.debug_compare(a, b, nbytes, f2, 2, 1), vr.compare_flags(a, b, nbytes, f2, 2, 1)), (units, what, hex(fill))


class Launch:
    """one launch of a scan check kernel: items laid out in an `out` and a `ref` arena of random bytes, each with the answer the case expects"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.out, self.ref = bytearray(), bytearray()
        self.items, self.lens, self.differs, self.what = [], [], [], []

    def _place(self, arena, mod, data):
        arena += bytes(self.rng.integers(0, 256, (-len(arena)) % 16 + 16 + mod, dtype=np.uint8))   # a guard, then the alignment asked for
        assert len(arena) % 16 == mod
        arena += data
        return len(arena) - len(data)

    def add(self, what, ref_len, differs, flip_out=None, flip_ref=None, out_len=None, image=None, prefix=False, out_mod=0, ref_mod=0):
        """an item of ref_len equal bytes (16 more behind them, equal too), then one byte flipped in `out` and / or in `ref` at the index
        given (ref_len itself is the byte behind the item).  image None: a flag word of its own"""
        data = bytearray(self.rng.integers(0, 256, ref_len + 16, dtype=np.uint8).tobytes())
        o, r = bytearray(data), bytearray(data)
        if flip_out is not None:
            assert 0 <= flip_out < ref_len + 16
            o[flip_out] ^= 1 << int(self.rng.integers(0, 8))
        if flip_ref is not None:
            assert 0 <= flip_ref < ref_len + 16
            r[flip_ref] ^= 1 << int(self.rng.integers(0, 8))
        oo, ro = self._place(self.out, out_mod, o), self._place(self.ref, ref_mod, r)
        image = len(self.items) if image is None else image
        self.items.append((oo, ro, ref_len, image | (vr.PREFIX if prefix else 0)))
        self.lens.append(ref_len if out_len is None else out_len)
        self.differs.append(differs)
        self.what.append(what)

    def add_flips(self, ref_len, **kw):
        """the byte positions at which a check of ref_len bytes can go wrong, one item each"""
        whole = ref_len // 16 * 16
        self.add("%d equal" % ref_len, ref_len, False, **kw)
        if ref_len:
            self.add("%d byte 0" % ref_len, ref_len, True, flip_out=0, **kw)
            self.add("%d last byte" % ref_len, ref_len, True, flip_out=ref_len - 1, **kw)
            self.add("%d last byte, in ref" % ref_len, ref_len, True, flip_ref=ref_len - 1, **kw)
        if whole:
            self.add("%d last byte of the last whole unit" % ref_len, ref_len, True, flip_out=whole - 1, **kw)
        if ref_len > whole:
            self.add("%d first tail byte" % ref_len, ref_len, True, flip_out=whole, **kw)
        self.add("%d the byte behind, in out" % ref_len, ref_len, False, flip_out=ref_len, **kw)
        self.add("%d the byte behind, in ref" % ref_len, ref_len, False, flip_ref=ref_len, **kw)

    def add_lengths(self, ref_len, bytes_form, **kw):
        """the written length against ref_len, bytes equal"""
        self.add("%d written one more" % ref_len, ref_len, True, out_len=ref_len + 1, **kw)
        if ref_len:
            self.add("%d written one less" % ref_len, ref_len, True, out_len=ref_len - 1, **kw)
        self.add("%d the writer gave up (bit 31)" % ref_len, ref_len, True, out_len=ref_len | 0x80000000, **kw)
        if bytes_form:
            return
        self.add("%d prefix, as long" % ref_len, ref_len, False, prefix=True, **kw)
        self.add("%d prefix, longer" % ref_len, ref_len, False, out_len=ref_len + 77, prefix=True, **kw)
        self.add("%d prefix, longer, bit 31" % ref_len, ref_len, False, out_len=(ref_len + 1) | 0x80000000, prefix=True, **kw)
        self.add("%d prefix, as long, bit 31" % ref_len, ref_len, False, out_len=ref_len | 0x80000000, prefix=True, **kw)
        if ref_len:
            self.add("%d prefix, shorter" % ref_len, ref_len, True, out_len=ref_len - 1, prefix=True, **kw)
            self.add("%d prefix, shorter, bit 31" % ref_len, ref_len, True, out_len=(ref_len - 1) | 0x80000000, prefix=True, **kw)
            self.add("%d prefix, longer, last byte differs" % ref_len, ref_len, True, out_len=ref_len + 3, prefix=True, flip_out=ref_len - 1, **kw)
            self.add("%d prefix, longer, the byte behind differs" % ref_len, ref_len, False, out_len=ref_len + 3, prefix=True, flip_out=ref_len, **kw)

    def run(self, codec, bytes_form, nflags=None, fill=SCAN_FILL):
        out = np.frombuffer(bytes(self.out) + bytes(32), dtype=np.uint8)
        ref = np.frombuffer(bytes(self.ref) + bytes(32), dtype=np.uint8)
        flags = np.full((nflags or len(self.items)) + 5, fill, dtype=np.uint32)
        for it, n, differs, what in zip(self.items, self.lens, self.differs, self.what):
            assert vr.scan_item_differs(out, n, ref, it, bytes_form) == differs, what
        want = vr.scan_check_flags(out, self.lens, ref, self.items, flags, bytes_form)
        got = codec.debug_scan_check(bytes_form, out, self.lens, ref, self.items, flags)
        wrong = [(self.what[i], hex(got[it[3] & ~vr.PREFIX])) for i, it in enumerate(self.items) if got[it[3] & ~vr.PREFIX] != want[it[3] & ~vr.PREFIX]]
        assert not wrong, wrong[:8]
        assert np.array_equal(got, want)
        return got


SCAN_LENGTHS = list(range(49)) + [4095, 4096, 4097]


def test_scan_check_kernel_byte_positions(gpu_codec):
    """lep_scan_check_kernel, both arenas 16-byte aligned: every ref_len from 0 to 48, then around 4096 -- one launch, one flag word per item"""
    run = Launch(1)
    for n in SCAN_LENGTHS:
        run.add_flips(n)
    got = run.run(gpu_codec, False)
    assert sum(run.differs) > 150 and len(run.differs) - sum(run.differs) > 150
    assert (got[len(run.items):] == SCAN_FILL).all()
    for fill in (0xFFFFFFFF, 0xFFFFFFFD, 2):     # bits that were set stay set
        run.run(gpu_codec, False, fill=fill)


def test_scan_check_kernel_length_field(gpu_codec):
    run = Launch(2)
    for n in (0, 1, 15, 16, 17, 37, 4096, 4097):
        run.add_lengths(n, False)
    run.run(gpu_codec, False)
    assert any(run.differs) and not all(run.differs)


def test_scan_checks_share_flag_words_by_image(gpu_codec):
    """several items naming the same image and different images in one launch: only the image whose item differs gets bit 1"""
    for bytes_form in (False, True):
        mods = dict(out_mod=5, ref_mod=11) if bytes_form else {}
        run = Launch(3)
        for image, flip in [(0, None), (0, None), (2, None), (2, 20), (2, None), (4, 0), (4, 36), (1, None), (6, None), (0, None)]:
            run.add("image %d" % image, 37, flip is not None, flip_out=flip, image=image, **mods)
        if not bytes_form:
            run.add("image 3, prefix", 37, False, out_len=50, image=3, prefix=True)
            run.add("image 5, prefix, shorter", 37, True, out_len=36, image=5, prefix=True)
            run.add("image 5", 37, False, image=5)
        got = run.run(gpu_codec, bytes_form, nflags=8)
        want_set = {2, 4} | (set() if bytes_form else {5})
        assert [int(v) for v in got] == [SCAN_FILL | (2 if i in want_set else 0) for i in range(len(got))]


def test_scan_check_bytes_kernel_every_alignment(gpu_codec):
    """lep_scan_check_bytes_kernel: all 16 x 16 pairs of out_off mod 16, ref_off mod 16 at ref_len 37"""
    run = Launch(4)
    for om in range(16):
        for rm in range(16):
            kw = dict(out_mod=om, ref_mod=rm)
            run.add("(%d, %d) equal" % (om, rm), 37, False, **kw)
            run.add("(%d, %d) byte 0" % (om, rm), 37, True, flip_out=0, **kw)
            run.add("(%d, %d) last byte" % (om, rm), 37, True, flip_ref=36, **kw)
            run.add("(%d, %d) the byte behind" % (om, rm), 37, False, flip_out=37, **kw)
    got = run.run(gpu_codec, True)
    assert len(run.items) == 1024 and (got[1024:] == SCAN_FILL).all()


def test_scan_check_bytes_kernel_lengths(gpu_codec):
    """... and ref_len 0, 1, 255, 256, 257, 1025 at one odd pair of offsets: the byte positions, then the written length"""
    run = Launch(5)
    for n in (0, 1, 255, 256, 257, 1025):
        run.add_flips(n, out_mod=3, ref_mod=9)
        run.add_lengths(n, True, out_mod=3, ref_mod=9)
    run.run(gpu_codec, True)
    for fill in (0xFFFFFFFF, 0xFFFFFFFD, 2):
        run.run(gpu_codec, True, fill=fill)


def test_debug_entry_points_refuse_what_the_kernels_cannot_take(gpu_codec):
    from lepton_amd.codec import LeptonError

    buf = np.zeros(64, dtype=np.uint8)
    flags = np.zeros(2, dtype=np.uint32)
    with pytest.raises(LeptonError):      # the aligned form on an offset that is not aligned
        gpu_codec.debug_scan_check(False, buf, [8], buf, [(4, 0, 8, 0)], flags)
    with pytest.raises(LeptonError):      # the bytes form takes no prefix item
        gpu_codec.debug_scan_check(True, buf, [8], buf, [(0, 0, 8, vr.PREFIX)], flags)
    with pytest.raises(ValueError):       # an item that leaves the arrays never reaches the library
        gpu_codec.debug_scan_check(True, buf, [8], buf, [(60, 0, 8, 0)], flags)
    with pytest.raises(ValueError):
        gpu_codec.debug_scan_check(True, buf, [8], buf, [(0, 0, 8, 2)], flags)
    assert np.array_equal(gpu_codec.debug_scan_check(True, buf, [], buf, [], flags), flags)
