"""The kernel headers (lepton_amd/csrc/*.h; and the single-lane coder tests/emu/lep_core_coder.h) compiled with g++ and single-stepped on the CPU
(tests/emu/core_emu.cc) must produce the oracle's streams and frames.  Catches logic errors in the
device code without a GPU; the real GPU parity tests are in test_gpu_parity.py."""
import ctypes as C
import os
import subprocess

import pytest

import oracle_binding as ob
from conftest import ROOT, golden, golden_cases
from lepton_amd.codec import JpegImage

def _host_path(jpg, want_lep=None, restored=None):
    """what the product does with a file a kernel leaves alone: the host parser + the oracle write the .lep (the reference's bytes, where
    the fixture has them) and the host re-coder restores from it the file -- or, for a damaged one, what the reference restores"""
    import hashlib
    from lepton_amd.codec import LepFile

    img = JpegImage(jpg)
    streams, _ = ob.oracle_encode(img.desc, img.plan())
    lep = img.write_lep(streams)
    if want_lep is not None:
        assert lep == want_lep, "the host path's .lep differs from the reference's"
    f = LepFile(lep)
    ob.oracle_decode(f.desc, f.segments, f.streams)
    back = f.recode()
    assert back == jpg if restored is None else hashlib.md5(back).hexdigest() == restored, "the host path does not restore the file"


def _golden_lep(name):
    """the reference's .lep of a named fixture (tests/golden, tests/golden/ref), None for a generated file"""
    from conftest import GOLDEN, REF_GOLDEN

    for d in (GOLDEN, REF_GOLDEN):
        p = os.path.join(d, name + ".lep")
        if os.path.exists(p):
            return open(p, "rb").read()
    return None


EMU_SO = os.environ.get("LEP_EMU_SO") or os.path.join(ROOT, "tests", "emu", "libcore_emu.so")   # LEP_EMU_SO: sanitizer builds go elsewhere


@pytest.fixture(scope="module")
def emu():
    src = os.path.join(ROOT, "tests", "emu", "core_emu.cc")
    extra = os.environ.get("LEP_EMU_DEFINES", "").split()   # experiment variants of the kernels (-DLEP_...)
    tmp = "%s.%d" % (EMU_SO, os.getpid())    # (several pytest-xdist workers may build it at once: write aside, rename into place)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared"] + extra + ["-o", tmp, src])
    os.replace(tmp, EMU_SO)
    return C.CDLL(EMU_SO)


@pytest.fixture(scope="module")
def emu_other_forms():
    """the v4 decoder with the OTHER assignment of its serial rounds to the scalar / vector unit (lep_dec4.h LEP_DEC4_SCALAR:
    the shipped build runs the 7x7 round on the scalar unit, this one everything but): every round is stepped in both forms"""
    src = os.path.join(ROOT, "tests", "emu", "core_emu.cc")
    so = os.path.join(ROOT, "tests", "emu", "libcore_emu_forms.so")
    tmp = "%s.%d" % (so, os.getpid())
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-DLEP_DEC4_SCALAR=13", "-o", tmp, src])
    os.replace(tmp, so)
    return C.CDLL(so)


@pytest.mark.parametrize("name", golden_cases())
def test_kernel_source_on_cpu_matches_oracle(emu, name):
    jpg, _ = golden(name)
    img = JpegImage(jpg)
    d = img.desc
    segs = img.plan()
    want, bins = ob.oracle_encode(d, segs)
    for s, w in zip(segs, want):
        cap = len(w) + 4096
        buf = C.create_string_buffer(cap)
        n, nb = C.c_uint32(0), C.c_uint32(0)
        rc = emu.emu_encode_segment(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, buf, cap, C.byref(n), C.byref(nb))
        assert rc == 0 and buf.raw[: n.value] == w
    orig = [C.string_at(d.blocks[c], d.nblocks(c) * 128) for c in range(d.ncomp)]
    for c in range(d.ncomp):
        C.memset(d.blocks[c], 0, d.nblocks(c) * 128)
    for s, w in zip(segs, want):
        assert emu.emu_decode_segment(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, w, len(w), None) == 0
    for c in range(d.ncomp):
        n = d.coded_blocks[c] * 128
        assert C.string_at(d.blocks[c], n) == orig[c][:n]


@pytest.mark.parametrize("gen", ["v4"])
@pytest.mark.parametrize("name", golden_cases())
def test_v3_decoder_on_cpu_matches_oracle(emu, name, gen):
    """lep_dec4.h as 64-lane loop emulations: decoding the oracle's streams returns the coefficient frame and
    consumes exactly the oracle's number of bins"""
    jpg, _ = golden(name)
    img = JpegImage(jpg)
    d = img.desc
    segs = img.plan()
    want, bins = ob.oracle_encode(d, segs)
    orig = [C.string_at(d.blocks[c], d.nblocks(c) * 128) for c in range(d.ncomp)]
    for c in range(d.ncomp):
        C.memset(d.blocks[c], 0, d.nblocks(c) * 128)
    total = 0
    for s, w in zip(segs, want):
        nb = C.c_uint32(0)
        assert getattr(emu, "emu_decode_segment_" + gen)(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, w, len(w), C.byref(nb)) == 0
        total += nb.value
    assert total == bins
    for c in range(d.ncomp):
        n = d.coded_blocks[c] * 128
        assert C.string_at(d.blocks[c], n) == orig[c][:n]


@pytest.mark.parametrize("gen", ["v4"])
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_v3_decoder_unaligned_stream_start(emu, shift, gen):
    """the 64-bit window reads aligned dwords only: a stream that starts 1..3 bytes into a dword (streams packed back to
    back in the arena) and ends mid-dword must decode exactly like an aligned one, never touching bytes outside it"""
    jpg, _ = golden("c420_odd_203x149")
    img = JpegImage(jpg)
    d = img.desc
    segs = img.plan()
    want, bins = ob.oracle_encode(d, segs)
    orig = [C.string_at(d.blocks[c], d.nblocks(c) * 128) for c in range(d.ncomp)]
    for c in range(d.ncomp):
        C.memset(d.blocks[c], 0, d.nblocks(c) * 128)
    for s, w in zip(segs, want):
        arena = C.create_string_buffer(b"\xff" * 8 + b"\xa5" * shift + w + b"\x5a" * 9)   # poison either side
        base = C.addressof(arena)
        base += (-base) % 4 + 4   # a 4-aligned address inside the poison prefix ...
        C.memmove(base + shift, w, len(w))   # ... so the stream itself starts `shift` bytes into a dword
        C.memset(base, 0xA5, shift)
        C.memset(base + shift + len(w), 0x5A, 8)
        assert getattr(emu, "emu_decode_segment_" + gen)(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, C.c_void_p(base + shift), len(w), None) == 0
    for c in range(d.ncomp):
        n = d.coded_blocks[c] * 128
        assert C.string_at(d.blocks[c], n) == orig[c][:n]


@pytest.fixture(params=["one wavefront", "producer + consumer"])
def enc_mode(request, monkeypatch):
    """the encoder's two forms: one wavefront per segment, or the producer half of the two-wave kernel handing its bin-list
    chunks through the double buffer (the emulation runs the consumer's step in place)"""
    if request.param != "one wavefront":
        monkeypatch.setenv("LEP_EMU_ENC_PIPE", "1")
    else:
        monkeypatch.delenv("LEP_EMU_ENC_PIPE", raising=False)
    return request.param


@pytest.mark.parametrize("name", golden_cases())
def test_v3_encoder_on_cpu_matches_oracle(emu, name, enc_mode):
    """lep_enc3.h (lane-range bin list, uniform-vector bool coder) as a 64-lane loop emulation == oracle streams"""
    jpg, _ = golden(name)
    img = JpegImage(jpg)
    d = img.desc
    segs = img.plan()
    want, bins = ob.oracle_encode(d, segs)
    total = 0
    for s, w in zip(segs, want):
        cap = len(w) + 4096
        buf = C.create_string_buffer(cap)
        n, nb = C.c_uint32(0), C.c_uint32(0)
        rc = emu.emu_encode_segment_v3(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, buf, cap, C.byref(n), C.byref(nb))
        assert rc == 0 and buf.raw[: n.value] == w
        total += nb.value
    assert total == bins


def test_v3_encoder_many_bins_per_block(emu, enc_mode):
    """blocks whose bin list does not fit one 512-entry lane range (large coefficients everywhere) are coded in several
    ranges; streams must still equal the oracle's, and out-of-range coefficients are reported like the reference does"""
    import numpy as np
    from lepton_amd import corpus

    img = JpegImage(corpus.synth_jpeg(64, 48, 11, quality=100))
    d = img.desc
    rng = np.random.default_rng(5)
    for c in range(d.ncomp):
        n = d.nblocks(c) * 64
        arr = (C.c_int16 * n).from_address(d.blocks[c])
        vals = rng.integers(-255, 256, n)
        vals[rng.random(n) < 0.1] = 0
        for i in range(n):
            arr[i] = int(vals[i])
        for b in range(d.nblocks(c)):
            arr[b * 64 + 49] = 0
    segs = img.plan()
    want, bins = ob.oracle_encode(d, segs)
    assert bins > 560 * sum(d.nblocks(c) for c in range(d.ncomp))   # really > 512 bins per block
    for s, w in zip(segs, want):
        cap = len(w) + 4096
        buf = C.create_string_buffer(cap)
        n = C.c_uint32(0)
        rc = emu.emu_encode_segment_v3(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, buf, cap, C.byref(n), None)
        assert rc == 0 and buf.raw[: n.value] == w
    C.cast(d.blocks[0], C.POINTER(C.c_int16))[5] = 4096
    s = segs[0]
    buf = C.create_string_buffer(1 << 20)
    n = C.c_uint32(0)
    assert emu.emu_encode_segment_v3(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, buf, len(buf), C.byref(n), None) == 6


@pytest.mark.parametrize("gen", ["v4"])
def test_v4_decoder_large_coefficients(emu, gen):
    """every rare path of lep_dec4.h at once: exponent bins beyond the prefetched groups, residual bits >= 4, threshold
    bins, long interior runs (several windows, all non-zero bins)"""
    import numpy as np
    from lepton_amd import corpus

    img = JpegImage(corpus.synth_jpeg(64, 48, 11, quality=100))
    d = img.desc
    rng = np.random.default_rng(5)
    for c in range(d.ncomp):
        n = d.nblocks(c) * 64
        arr = (C.c_int16 * n).from_address(d.blocks[c])
        vals = rng.integers(-255, 256, n)
        vals[rng.random(n) < 0.1] = 0
        for i in range(n):
            arr[i] = int(vals[i])
        for b in range(d.nblocks(c)):
            arr[b * 64 + 49] = 0
    segs = img.plan()
    want, bins = ob.oracle_encode(d, segs)
    orig = [C.string_at(d.blocks[c], d.nblocks(c) * 128) for c in range(d.ncomp)]
    for c in range(d.ncomp):
        C.memset(d.blocks[c], 0, d.nblocks(c) * 128)
    total = 0
    for s, w in zip(segs, want):
        nb = C.c_uint32(0)
        assert getattr(emu, "emu_decode_segment_" + gen)(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, w, len(w), C.byref(nb)) == 0
        total += nb.value
    assert total == bins
    for c in range(d.ncomp):
        n = d.coded_blocks[c] * 128
        assert C.string_at(d.blocks[c], n) == orig[c][:n]


def test_v4_decoder_rounds_in_their_other_form(emu_other_forms):
    """scalar-unit and vector-unit forms of every serial round decode the same frames: golden cases, the rare paths
    (large coefficients), garbage streams"""
    emu = emu_other_forms
    for name in golden_cases():
        jpg, _ = golden(name)
        img = JpegImage(jpg)
        d = img.desc
        segs = img.plan()
        want, bins = ob.oracle_encode(d, segs)
        orig = [C.string_at(d.blocks[c], d.nblocks(c) * 128) for c in range(d.ncomp)]
        for c in range(d.ncomp):
            C.memset(d.blocks[c], 0, d.nblocks(c) * 128)
        for gen in ("v4",):
            for c in range(d.ncomp):
                C.memset(d.blocks[c], 0, d.nblocks(c) * 128)
            total = 0
            for s, w in zip(segs, want):
                nb = C.c_uint32(0)
                assert getattr(emu, "emu_decode_segment_" + gen)(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, w, len(w), C.byref(nb)) == 0, name
                total += nb.value
            assert total == bins, name
            for c in range(d.ncomp):
                n = d.coded_blocks[c] * 128
                assert C.string_at(d.blocks[c], n) == orig[c][:n], name
    test_v4_decoder_large_coefficients(emu, "v4")
    test_decoders_survive_garbage_streams(emu, 9)


def test_inv24_table_update_is_exact(emu):
    """lep_dec4.h's Branch update (24-bit table reciprocal, v_mul_u32_u24) == branch.hh:82-100 for every count pair,
    both observations, saturation and halving paths included"""
    assert emu.emu_check_inv24_update() == 0


def test_division_by_multiplication_is_exact(emu):
    """lep_dec4.h divides by a row's constants (the Lakhani divisors, the DC quantiser) with one multiplication: every divisor the tables
    can hold, numerators at the multiples of the divisor +- 1, the extremes, random ones"""
    assert emu.emu_check_div_by() == 0


@pytest.mark.parametrize("name", golden_cases())
def test_gpu_huffman_encoder_on_cpu_restores_the_jpeg(emu, name):
    """lep_huff.h (wave-cooperative JPEG Huffman re-encode) as a 64-lane loop emulation: for every eligible fixture the
    segments' scan bytes glued by recode_finish == the original JPEG == what the host re-encoder produces"""
    from lepton_amd import abi
    from lepton_amd.codec import LepFile

    jpg, lep = golden(name)
    L = abi.lib()
    f = LepFile(lep)
    src = JpegImage(jpg)          # coefficient frame from the JPEG itself (what the arithmetic decoder would restore)
    for c in range(f.desc.ncomp):
        C.memmove(f.desc.blocks[c], src.desc.blocks[c], f.desc.nblocks(c) * 128)
    assert f.recode() == jpg      # host path
    img = abi.HuffImage()
    segs = (abi.HuffSegment * abi.MAX_SEGMENTS)()
    nseg, ok = C.c_int(0), C.c_int(0)
    assert L.lep_file_recode_plan(f.handle, C.byref(img), segs, C.byref(nseg), C.byref(ok)) == 0
    if not ok.value:   # not for the GPU Huffman encoder (truncated file, legacy hand-offs, ...): the host re-coder above is the product's path
        assert nseg.value == 0
        return
    outs = (abi.Bytes * nseg.value)()
    ends = (abi.HuffEnd * nseg.value)()
    keep = []
    for i in range(nseg.value):
        cap = min(segs[i].out_cap, len(jpg) + 1024)
        segs[i].out_cap = cap
        buf = C.create_string_buffer(cap + 8)
        keep.append(buf)
        n = C.c_uint32(0)
        assert emu.emu_huffman_encode_segment(C.byref(img), C.byref(segs[i]), buf, C.byref(n), C.byref(ends[i])) == 0
        outs[i].data = C.cast(buf, C.c_void_p).value
        outs[i].len = outs[i].cap = n.value
    out = abi.Bytes()
    assert L.lep_file_recode_finish(f.handle, outs, ends, nseg.value, C.byref(out)) == 0
    got = out.tobytes()
    L.lep_free(out.data)
    assert got == jpg


@pytest.mark.parametrize("name", golden_cases() + ["synth_1280x720", "synth_q100", "optimized_q30", "optimized_q95", "optimized_noise_444"])
def test_lane_per_unit_huffman_encoder_equals_the_wave_per_segment_one(emu, name):
    """lep_huff_simt.h (one lane per run of eight MCUs: count, prefix sums, bits OR-ed into the segment's bit buffer, stuffing pass)
    must write what lep_huff.h writes -- the segment's bytes, its byte count under a bound, the end state the next hand-off is held
    against -- or leave the segment to it (restart intervals, non-interleaved scans)"""
    from lepton_amd import abi, corpus
    from lepton_amd.codec import LepFile, GpuCodec

    if name.startswith("synth") or name.startswith("optimized"):
        jpg = (corpus.synth_jpeg(1280, 720, 81, quality=92) if name == "synth_1280x720" else corpus.synth_jpeg(320, 240, 82, quality=100)) if name.startswith("synth") else _jpeg_for_huffman_tests(name)
        import oracle_binding as ob
        img0 = JpegImage(jpg)
        segs0 = img0.plan()
        streams, _ = ob.oracle_encode(img0.desc, segs0)
        lep = img0.write_lep(streams)
    else:
        jpg, lep = golden(name)
    L = abi.lib()
    f = LepFile(lep)
    src = JpegImage(jpg)
    for c in range(f.desc.ncomp):
        C.memmove(f.desc.blocks[c], src.desc.blocks[c], f.desc.nblocks(c) * 128)
    img = abi.HuffImage()
    segs = (abi.HuffSegment * abi.MAX_SEGMENTS)()
    nseg, ok = C.c_int(0), C.c_int(0)
    assert L.lep_file_recode_plan(f.handle, C.byref(img), segs, C.byref(nseg), C.byref(ok)) == 0
    if not ok.value:   # not for the GPU Huffman encoder: the host re-coder restores it
        assert nseg.value == 0 and f.recode() == jpg
        return
    if any(img.trunc_bc[c] for c in range(4)):   # a file cut inside its scan: only the lane-per-unit kernels know the cut
        assert f.recode() == jpg                  # (test_..._restores_files_cut_inside_their_scan); here the host re-coder's bytes
        return
    taken = 0
    for i in range(nseg.value):
        for cap in (min(segs[i].out_cap, len(jpg) + 1024), 100):        # the segment's own bound, and one that cuts it short
            segs[i].out_cap = cap
            outs = []
            for fn in (emu.emu_huffman_encode_segment, emu.emu_huffman_encode_segment_simt):
                buf = C.create_string_buffer(cap + 8)
                n = C.c_uint32(0)
                end = abi.HuffEnd()
                rc = fn(C.byref(img), C.byref(segs[i]), buf, C.byref(n), C.byref(end))
                outs.append((rc, n.value, buf.raw[: n.value], end.overhang_byte, end.num_overhang_bits, list(end.last_dc)))
            if outs[1][0] == 1:
                continue
            taken += 1
            assert outs[0] == outs[1], (i, cap, outs[0][1], outs[1][1], outs[0][3:], outs[1][3:])
    if img.interleaved and img.ncomp >= 2:
        assert taken > 0          # (restart intervals too, since round 5)


@pytest.mark.parametrize("name", golden_cases() + ["synth_640x360", "synth_rst", "optimized_q95", "optimized_q30", "optimized_noise_444"])
def test_gpu_huffman_decoder_on_cpu_matches_host_parser(emu, name):
    """lep_huffdec.h (wave-per-image JPEG Huffman scan decode) as a 64-lane loop emulation + parse_jpeg_finish_gpu: for
    every eligible file the coefficient frame, the hand-off records and the pad bit equal the host parser's, so the .lep
    written from them is the reference's"""
    import io
    from lepton_amd import abi, corpus

    if name == "synth_640x360":
        jpg = corpus.synth_jpeg(640, 360, 71, quality=88)
    elif name.startswith("optimized"):
        # per-image Huffman tables (libjpeg optimize_coding): code lengths differ from the Annex K tables, long DC codes,
        # rare symbols with 14..16-bit codes -- the kernel's long-code path (canonical test across lanes)
        from PIL import Image
        import numpy as np
        rng = np.random.default_rng(31)
        if name == "optimized_noise_444":
            a = rng.integers(0, 256, (120, 168, 3), dtype=np.uint8)
            q, sub = 98, "4:4:4"
        else:
            base = rng.integers(0, 256, (30, 40, 3), dtype=np.uint8)
            a = np.asarray(Image.fromarray(base, "RGB").resize((320, 240), Image.BICUBIC)).astype(np.int16)
            a = np.clip(a + rng.normal(0, 12, a.shape), 0, 255).astype(np.uint8)
            q, sub = (95, "4:2:0") if name.endswith("95") else (30, "4:2:2")
        buf = io.BytesIO(); Image.fromarray(a, "RGB").save(buf, format="JPEG", quality=q, subsampling=sub, optimize=True)
        jpg = buf.getvalue()
    elif name == "synth_rst":
        from PIL import Image
        import numpy as np
        rng = np.random.default_rng(9)
        im = Image.fromarray(rng.integers(0, 256, (96, 160, 3), dtype=np.uint8), "RGB")
        buf = io.BytesIO(); im.save(buf, format="JPEG", quality=70, subsampling="4:2:0", restart_marker_blocks=3)
        jpg = buf.getvalue()
    else:
        jpg, _ = golden(name)
    L = abi.lib()
    host = JpegImage(jpg)
    h = C.c_void_p()
    img = abi.HuffDecImage()
    ok = C.c_int(0)
    rc = L.lep_jpeg_open_gpu(jpg, len(jpg), C.byref(h), C.byref(img), C.byref(ok))
    assert rc == 0
    if not ok.value or img.flags & 1:
        # not for the GPU Huffman decoder (grey, multi-scan, ...), or a file cut inside its scan (the single-wave kernel reports it
        # irregular, the lane-per-subsequence kernels decode it): the host parser's path must give the reference's .lep and restore it
        L.lep_jpeg_close(h)
        _host_path(jpg, _golden_lep(name))
        return
    p, n = C.c_void_p(), C.c_size_t(0)
    L.lep_jpeg_scan_bytes(h, C.byref(p), C.byref(n))
    scan = C.create_string_buffer(C.string_at(p, n.value) + b"\0" * 64, n.value + 64)   # zero padded copy ("device" arena)
    base = C.addressof(scan)
    assert base % 8 == 0
    img.scan = base
    d = host.desc
    planes = []
    for c in range(d.ncomp):
        b = C.create_string_buffer(d.nblocks(c) * 128)
        planes.append(b)
        img.blocks[c] = C.cast(b, C.c_void_p).value
    rows = (abi.HuffDecRow * (img.mcuv + 1))()
    assert emu.emu_huffman_decode_image(C.byref(img), rows) == 0
    assert rows[img.mcuv].aux >> 8 == 0, "kernel reported an irregular scan on a clean fixture"
    for c in range(d.ncomp):
        assert planes[c].raw == C.string_at(d.blocks[c], d.nblocks(c) * 128)
    assert L.lep_jpeg_finish_gpu(h, rows) == 0
    # the container written from the GPU-side parse == the one from the host parse (== the reference's for the fixtures)
    segs = host.plan()
    streams, _ = ob.oracle_encode(d, segs)
    want = host.write_lep(streams)
    arr = (abi.Bytes * len(streams))()
    keep = []
    for i, s in enumerate(streams):
        b = C.create_string_buffer(bytes(s), max(1, len(s)))
        keep.append(b)
        arr[i].data = C.cast(b, C.c_void_p).value
        arr[i].len = arr[i].cap = len(s)
    out = abi.Bytes()
    assert L.lep_jpeg_write_lep(h, 0, arr, len(streams), C.byref(out)) == 0
    got = out.tobytes()
    L.lep_free(out.data)
    L.lep_jpeg_close(h)
    assert got == want


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_decoders_survive_garbage_streams(emu, seed):
    """corrupt / random arithmetic-coded streams must make the decoder kernels return (0 or an exit code such as
    STREAM_INCONSISTENT) -- never loop or index outside the model / frame: a hang on the GPU box would take the node down"""
    import numpy as np
    from lepton_amd import corpus

    img = JpegImage(corpus.synth_jpeg(96, 64, 77))
    d = img.desc
    segs = img.plan()
    rng = np.random.default_rng(seed)
    for fn in ("emu_decode_segment_v4", "emu_decode_segment"):
        for kind in range(3):
            n = int(rng.integers(0, 400))
            if kind == 0:
                data = bytes(rng.integers(0, 256, n, dtype=np.uint8))
            elif kind == 1:
                data = bytes([255]) * n
            else:
                data = bytes(n)
            for c in range(d.ncomp):
                C.memset(d.blocks[c], 0, d.nblocks(c) * 128)
            s = segs[0]
            rc = getattr(emu, fn)(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, data, len(data), None)
            assert rc in (0, 6, 7, 43), (fn, kind, rc)


@pytest.mark.parametrize("seed", [4, 5])
def test_gpu_huffman_decoder_survives_garbage_scans(emu, seed):
    """random bytes in place of the entropy-coded scan: the Huffman decode kernel logic reports an irregular scan (or
    decodes garbage) but terminates and stays inside the scan / frame"""
    import numpy as np
    from lepton_amd import abi, corpus

    jpg = corpus.synth_jpeg(96, 64, 78)
    L = abi.lib()
    h = C.c_void_p()
    img = abi.HuffDecImage()
    ok = C.c_int(0)
    assert L.lep_jpeg_open_gpu(jpg, len(jpg), C.byref(h), C.byref(img), C.byref(ok)) == 0 and ok.value
    rng = np.random.default_rng(seed)
    n = img.scan_len
    scan = C.create_string_buffer(bytes(rng.integers(0, 256, n, dtype=np.uint8)) + bytes(64), n + 72)
    img.scan = C.addressof(scan)
    d = JpegImage(jpg).desc
    planes = [C.create_string_buffer(d.nblocks(c) * 128) for c in range(d.ncomp)]
    for c in range(d.ncomp):
        img.blocks[c] = C.cast(planes[c], C.c_void_p).value
    rows = (abi.HuffDecRow * (img.mcuv + 1))()
    assert emu.emu_huffman_decode_image(C.byref(img), rows) == 0
    if rows[img.mcuv].aux >> 8 == 0:
        assert L.lep_jpeg_finish_gpu(h, rows) in (0, 42)
    L.lep_jpeg_close(h)


@pytest.mark.parametrize("layout", ["444_one_pair", "two_one_pair", "y21_c_one_pair", "420_one_pair", "444_chroma_pair"])
def test_lane_per_subsequence_decoder_on_images_whose_blocks_share_their_tables(emu, layout):
    """When every block of the MCU is coded with the same DC and the same AC table, nothing in the bits tells a lane WHICH block of the MCU
    it stands on (lep_huffdec_simt.h simt_blind_phases): until round 6 such an image never settled -- the true position travels one lane per
    pass -- and went to the single-wave kernel after three wasted passes.  With 2 .. 4 blocks per MCU the lanes now sum DC differences per
    SLOT and pass P turns them into component sums once the prefix sum of block counts says where each lane stands: frame, records and
    status as the single-wave kernel leaves them, with subsequences far shorter than the product's so that every lane starts in mid-MCU."""
    import jpeg_writer as jw
    import numpy as np
    from lepton_amd import abi

    comps = {"444_one_pair": [(1, 1, 1, 0, 0, 0), (2, 1, 1, 0, 0, 0), (3, 1, 1, 0, 0, 0)],
             "two_one_pair": [(1, 1, 1, 0, 1, 1), (2, 1, 1, 0, 1, 1)],
             "y21_c_one_pair": [(1, 2, 1, 0, 0, 0), (2, 1, 1, 0, 0, 0)],
             "420_one_pair": [(1, 2, 2, 0, 0, 0), (2, 1, 1, 0, 0, 0), (3, 1, 1, 0, 0, 0)],          # six blocks per MCU: not taken, must still answer (or hand over)
             "444_chroma_pair": [(1, 1, 1, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)]}[layout]  # (the ordinary case: the tables tell the slots apart)
    settled = 0
    for w, h, dens, sub_bits in [(640, 480, 0.5, 4096), (333, 250, 0.1, 1024), (97, 50, 0.3, 512), (1300, 40, 0.1, 2048), (640, 480, 0.5, 32768)]:
        jpg, _ = jw.write_baseline(w, h, comps, np.random.default_rng(w * 7 + h), density=dens)
        one = _huffdec_setup(jpg)
        assert one is not None
        img, scan, planes, d = one
        rows1 = (abi.HuffDecRow * (img.mcuv + 1))()
        assert emu.emu_huffman_decode_image(C.byref(img), rows1) == 0 and rows1[img.mcuv].aux >> 8 == 0
        want = [p.raw for p in planes]
        for p in planes:
            C.memset(p, 0, len(p))
        rows2 = (abi.HuffDecRow * (img.mcuv + 1))()
        moved, nsub = (C.c_int32 * 8)(), C.c_uint32(0)
        assert emu.emu_huffman_decode_image_simt(C.byref(img), rows2, sub_bits, moved, C.byref(nsub)) == 0
        status = (rows2[img.mcuv].aux >> 8) & 0x3fffff
        if layout in ("420_one_pair", "444_chroma_pair") and status:
            continue                                                   # (the fallback's: a second chance with the single-wave kernel; subsequences this short need not settle)
        assert status == 0, (layout, w, h, sub_bits, status, list(moved)[:4], nsub.value)
        settled += 1
        assert [p.raw for p in planes] == want, (layout, w, h, sub_bits)
        assert [(r.bitpos, tuple(r.last_dc), r.aux) for r in rows2] == [(r.bitpos, tuple(r.last_dc), r.aux) for r in rows1], (layout, w, h, sub_bits)
        if nsub.value > 4 and layout.endswith("one_pair") and layout != "420_one_pair":   # (nothing travels lane by lane any more)
            assert not moved[2], (layout, w, h, "still moving in the second settle pass", list(moved)[:4])
    assert settled >= (5 if layout.endswith("one_pair") and layout != "420_one_pair" else 0)


def _huffdec_setup(jpg):
    """lep_jpeg_open_gpu + a zero padded copy of the scan + zeroed planes for the Huffman decode kernels' emulation"""
    from lepton_amd import abi

    L = abi.lib()
    h = C.c_void_p()
    img = abi.HuffDecImage()
    ok = C.c_int(0)
    assert L.lep_jpeg_open_gpu(jpg, len(jpg), C.byref(h), C.byref(img), C.byref(ok)) == 0
    if not ok.value:
        L.lep_jpeg_close(h)
        return None
    p, n = C.c_void_p(), C.c_size_t(0)
    L.lep_jpeg_scan_bytes(h, C.byref(p), C.byref(n))
    scan = C.create_string_buffer(C.string_at(p, n.value) + bytes(64), n.value + 64)
    img.scan = C.addressof(scan)
    d = JpegImage(jpg).desc
    planes = [C.create_string_buffer(d.nblocks(c) * 128) for c in range(d.ncomp)]
    for c in range(d.ncomp):
        img.blocks[c] = C.cast(planes[c], C.c_void_p).value
    L.lep_jpeg_close(h)
    return img, scan, planes, d



def _jpeg_for_huffman_tests(name):
    import io
    from lepton_amd import corpus
    if name == "synth_640x360":
        return corpus.synth_jpeg(640, 360, 71, quality=88)
    if name == "synth_1920x1080":
        return corpus.synth_jpeg(1920, 1080, 72, quality=90)
    if name in ("optimized_q30", "optimized_q95", "optimized_noise_444"):
        # per-image Huffman tables (libjpeg optimize_coding): long DC codes, rare symbols with 14..16-bit codes
        from PIL import Image
        import numpy as np
        rng = np.random.default_rng(31)
        if name == "optimized_noise_444":
            a = rng.integers(0, 256, (120, 168, 3), dtype=np.uint8)
            q, sub = 98, "4:4:4"
        else:
            a = np.asarray(Image.fromarray(rng.integers(0, 256, (30, 40, 3), dtype=np.uint8), "RGB").resize((320, 240), Image.BICUBIC)).astype(np.int16)
            a = np.clip(a + rng.normal(0, 12, a.shape), 0, 255).astype(np.uint8)
            q, sub = (95, "4:2:0") if name.endswith("95") else (30, "4:2:2")
        buf = io.BytesIO(); Image.fromarray(a, "RGB").save(buf, format="JPEG", quality=q, subsampling=sub, optimize=True)
        return buf.getvalue()
    return golden(name)[0]


@pytest.mark.parametrize("name", golden_cases() + ["synth_640x360", "synth_1920x1080", "optimized_q30", "optimized_q95", "optimized_noise_444"])
@pytest.mark.parametrize("sub_bits", [1024, 4096, 16384])
def test_lane_per_subsequence_huffman_decoder_equals_the_single_wave_one(emu, name, sub_bits):
    """lep_huffdec_simt.h (one lane per subsequence: a guess from the subsequence's first bit, settle passes from where the lane in front
    ended, prefix sums, write pass) must leave exactly what lep_huffdec.h leaves -- frame, hand-off records, pad bit -- or report a
    non-zero status (fallback), never a different result.  Subsequences far shorter than the product's 8192 bits are cut on purpose:
    then lanes do NOT fall into step inside their subsequence and the settle passes have work to do."""
    from lepton_amd import abi

    jpg = _jpeg_for_huffman_tests(name)
    one = _huffdec_setup(jpg)
    if one is None or one[0].rsti or one[0].flags & 1:
        # not for the GPU Huffman decoder; restart intervals (the single-wave kernel keeps these files); a file cut inside its scan (only
        # the lane-per-subsequence kernels know the cut: test_..._on_files_cut_inside_their_scan) -- the host parser's path is the product's
        if sub_bits == 1024:
            _host_path(jpg, _golden_lep(name))
        return
    img1, scan1, planes1, d = one
    rows1 = (abi.HuffDecRow * (img1.mcuv + 1))()
    assert emu.emu_huffman_decode_image(C.byref(img1), rows1) == 0 and rows1[img1.mcuv].aux >> 8 == 0
    img2, scan2, planes2, _ = _huffdec_setup(jpg)
    rows2 = (abi.HuffDecRow * (img2.mcuv + 1))()
    moved = (C.c_int32 * 8)()
    nsub = C.c_uint32(0)
    assert emu.emu_huffman_decode_image_simt(C.byref(img2), rows2, sub_bits, moved, C.byref(nsub)) == 0
    status = rows2[img2.mcuv].aux >> 8
    if status:
        # allowed only where the settle passes ran out: subsequences too short to fall into step in -- under 8192 bits, or under 64 of
        # the file's average block (the launch function gives such a file longer subsequences)
        blocks = sum(d.nblocks(c) for c in range(d.ncomp))
        assert (sub_bits < 8192 or sub_bits < 64 * img2.scan_len * 8 // blocks) and moved[3], "lane-per-subsequence decode gave up (status %d) with %d bits per subsequence, moved %s" % (status, sub_bits, list(moved)[:4])
        return
    assert not moved[3]
    for c in range(d.ncomp):
        assert planes2[c].raw == planes1[c].raw
    for r in range(img1.mcuv + 1):
        assert (rows2[r].bitpos, list(rows2[r].last_dc), rows2[r].aux) == (rows1[r].bitpos, list(rows1[r].last_dc), rows1[r].aux), r


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_lane_per_subsequence_huffman_decoder_survives_garbage(emu, seed):
    """random bytes instead of a scan: every pass terminates, nothing is written outside the frame, and the outcome is a status or
    (if the garbage happens to decode) the same as the single-wave kernel's"""
    import numpy as np
    from lepton_amd import abi, corpus

    jpg = corpus.synth_jpeg(96, 64, 78)
    outs = []
    for simt in (0, 1):
        img, scan, planes, d = _huffdec_setup(jpg)
        n = img.scan_len
        junk = C.create_string_buffer(bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)) + bytes(64), n + 72)
        img.scan = C.addressof(junk)
        rows = (abi.HuffDecRow * (img.mcuv + 1))()
        if simt:
            assert emu.emu_huffman_decode_image_simt(C.byref(img), rows, 1024, None, None) == 0
        else:
            assert emu.emu_huffman_decode_image(C.byref(img), rows) == 0
        outs.append((rows[img.mcuv].aux >> 8, [p.raw for p in planes]))
    if outs[0][0] == 0 and outs[1][0] == 0:
        assert outs[0][1] == outs[1][1]


def test_current_kernels_on_random_images_match_the_oracle(emu):
    """v3 encoder / v4 decoder kernel sources (lane-loop emulation) on seeded random JPEGs -- sizes from one block up, the
    chroma layouts PIL writes (4:4:4, 4:2:2, 4:2:0; the others are tests/test_sampling_layouts.py's), grey, qualities 5..100, flat to very noisy content,
    progressive and truncated files: streams equal the oracle's, frames come back (150 cases by hand, 25 here)"""
    import io
    import random
    import numpy as np
    from PIL import Image
    from lepton_amd.codec import LeptonError

    rnd = random.Random(11)
    done = 0
    for trial in range(25):
        w, h = rnd.choice([8, 17, 64, 97, 160, 333]), rnd.choice([8, 23, 48, 99, 240])
        mode = rnd.choice(["RGB", "RGB", "L"])
        rng = np.random.default_rng(9000 + trial)
        base = rng.integers(0, 256, (max(2, h // 8), max(2, w // 8), 3), dtype=np.uint8)
        a = np.asarray(Image.fromarray(base, "RGB").resize((w, h), rnd.choice([Image.BICUBIC, Image.NEAREST]))).astype(np.int16)
        amp = rnd.choice([0, 3, 12, 40, 120])
        a = np.clip(a + rng.normal(0, amp, a.shape) if amp else a, 0, 255).astype(np.uint8)
        kw = dict(format="JPEG", quality=rnd.choice([5, 20, 50, 75, 90, 97, 100]), progressive=rnd.random() < 0.3)
        if mode == "RGB":
            kw["subsampling"] = rnd.choice([0, 1, 2])
        buf = io.BytesIO()
        Image.fromarray(a, "RGB").convert(mode).save(buf, **kw)
        jpg = buf.getvalue()
        if rnd.random() < 0.15:
            jpg = jpg[: rnd.randint(len(jpg) // 2, len(jpg) - 1)]
        try:
            img = JpegImage(jpg)
        except LeptonError:
            continue
        d, segs = img.desc, img.plan()
        want, _ = ob.oracle_encode(d, segs)
        for s, wv in zip(segs, want):
            cap = len(wv) + 4096
            b = C.create_string_buffer(cap)
            n = C.c_uint32(0)
            assert emu.emu_encode_segment_v3(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, b, cap, C.byref(n), None) == 0
            assert b.raw[: n.value] == wv, trial
        for c in range(d.ncomp):
            C.memset(d.blocks[c], 0, d.nblocks(c) * 128)
        for s, wv in zip(segs, want):
            assert emu.emu_decode_segment_v4(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, wv, len(wv), None) == 0
        got = [C.string_at(d.blocks[c], d.nblocks(c) * 128) for c in range(d.ncomp)]
        for c in range(d.ncomp):
            C.memset(d.blocks[c], 0, d.nblocks(c) * 128)
        ob.oracle_decode(d, segs, want)
        assert got == [C.string_at(d.blocks[c], d.nblocks(c) * 128) for c in range(d.ncomp)], trial
        done += 1
    assert done >= 18


def _progressive_scans_on_the_emulation(emu, jpg, lep, simt=False, taken_out=None):
    """the frame of `jpg` through lep_huffprog.h's scan coders (lane-loop emulation), glued by the host; None if the file is
    not eligible for the GPU coder.  simt: through lep_huffprog_simt.h's lane-per-unit passes (and every scan held against the
    wavefront form's bytes)"""
    from lepton_amd import abi
    from lepton_amd.codec import LepFile

    L = abi.lib()
    f = LepFile(lep)
    src = JpegImage(jpg)
    for c in range(f.desc.ncomp):
        C.memmove(f.desc.blocks[c], src.desc.blocks[c], f.desc.nblocks(c) * 128)
    img = abi.HuffProgImage()
    scans = (abi.HuffProgScan * 64)()
    nscan, ok = C.c_int(0), C.c_int(0)
    assert L.lep_file_recode_plan_progressive(f.handle, C.byref(img), scans, 64, C.byref(nscan), C.byref(ok)) == 0
    if not ok.value:
        return None, f
    n = nscan.value
    out_total = corr_total = 0
    for i in range(n):
        scans[i].image = 0
        scans[i].out_off = out_total
        out_total += (scans[i].out_cap + 15) & ~15
        scans[i].corr_off = corr_total
        corr_total += scans[i].corr_cap
    out = C.create_string_buffer(out_total + 64)
    corr = (C.c_uint32 * (corr_total + 8))()
    lens = (C.c_uint32 * n)()
    emu.emu_huffman_progressive_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert emu.emu_huffman_progressive_encode(C.byref(img), scans, n, out, corr, lens) == 0
    assert all(l < 0x80000000 for l in lens), "a scan outgrew its slot"
    if simt:
        out2 = C.create_string_buffer(out_total + 64)
        lens2 = (C.c_uint32 * n)()
        taken = (C.c_int32 * n)()
        emu.emu_huffman_progressive_encode_simt.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        assert emu.emu_huffman_progressive_encode_simt(C.byref(img), scans, n, out2, corr, lens2, taken, 0) == 0
        for i in range(n):
            assert lens2[i] == lens[i], (i, lens2[i], lens[i], scans[i].from_, scans[i].to, scans[i].sah, scans[i].sal)
            a, b = scans[i].out_off, scans[i].out_off + lens[i]
            assert out2.raw[a:b] == out.raw[a:b], (i, scans[i].from_, scans[i].to, scans[i].sah, scans[i].sal)
        if taken_out is not None:
            taken_out.extend(taken)
        out, lens = out2, lens2
    sb = (abi.Bytes * n)()
    for i in range(n):
        sb[i].data = C.addressof(out) + scans[i].out_off
        sb[i].len = sb[i].cap = lens[i]
    res = abi.Bytes()
    assert L.lep_file_recode_finish_progressive(f.handle, sb, n, C.byref(res)) == 0
    data = res.tobytes()
    L.lep_free(res.data)
    return data, f


def _progressive_check_on_the_emulation(emu, jpg, tweak=None):
    """what lep_compress_batch's round-trip check does for a progressive file, with the scan coder stepped on the CPU: the plan
    from the PARSED file (lep_jpeg_plan_progressive_check), every scan written again from the parser's frame, compared with
    the file's own bytes of that scan.  None if the file is not eligible."""
    from lepton_amd import abi

    L = abi.lib()
    src = JpegImage(jpg)
    img = abi.HuffProgImage()
    scans = (abi.HuffProgScan * 64)()
    first = (C.c_uint32 * 64)()
    flen = (C.c_uint32 * 64)()
    nscan, ok = C.c_int(0), C.c_int(0)
    assert L.lep_jpeg_plan_progressive_check(src.handle, len(jpg), C.byref(img), scans, first, flen, 64, C.byref(nscan), C.byref(ok)) == 0
    if not ok.value:
        return None
    n = nscan.value
    for c in range(src.desc.ncomp):
        img.blocks[c] = src.desc.blocks[c]
    if tweak:
        tweak(src.desc)
    out_total = corr_total = 0
    for i in range(n):
        scans[i].image = 0
        scans[i].out_cap = min(scans[i].out_cap, flen[i] + 64)
        scans[i].out_off = out_total
        out_total += (scans[i].out_cap + 15) & ~15
        scans[i].corr_off = corr_total
        corr_total += scans[i].corr_cap
    out = C.create_string_buffer(out_total + 64)
    corr = (C.c_uint32 * (corr_total + 8))()
    lens = (C.c_uint32 * n)()
    emu.emu_huffman_progressive_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert emu.emu_huffman_progressive_encode(C.byref(img), scans, n, out, corr, lens) == 0
    return [(lens[i], out.raw[scans[i].out_off: scans[i].out_off + min(lens[i], scans[i].out_cap)], jpg[first[i]: first[i] + flen[i]]) for i in range(n)]


def test_progressive_round_trip_check_plan_on_cpu(emu):
    """every scan of the eligible progressive fixtures (and of random progressive files) comes back byte for byte from the plan
    the batch compressor's GPU round-trip check uses; a file whose scan bytes were altered does not"""
    from lepton_amd import corpus

    seen = 0
    files = [golden(n)[0] for n in golden_cases() if n.startswith("prog_")]
    files += [corpus.synth_jpeg(160, 120, 501, progressive=True), corpus.synth_jpeg(203, 149, 502, progressive=True, subsampling="4:4:4", quality=95),
              corpus.synth_jpeg(96, 64, 503, progressive=True, quality=30, subsampling="4:2:2")]
    for jpg in files:
        res = _progressive_check_on_the_emulation(emu, jpg)
        if res is None:
            continue
        seen += 1
        for length, got, want in res:
            assert length == len(want) and got == want
    assert seen >= 4
    # and it notices a frame that is not the file's: one coefficient changed -> some scan no longer matches
    def tweak(d):
        arr = (C.c_int16 * 64).from_address(d.blocks[0] + 128 * 3)
        arr[2] = arr[2] + 4 if arr[2] >= 0 else arr[2] - 4
    res = _progressive_check_on_the_emulation(emu, files[-3], tweak)
    assert res is not None and any(l != len(w) or g != w for l, g, w in res)


@pytest.mark.parametrize("name", [n for n in golden_cases() if n.startswith("prog_")])
def test_gpu_progressive_scan_encoder_on_cpu_restores_the_jpeg(emu, name):
    """lep_huffprog.h (DC / AC first-stage and refinement scans, end-of-band runs, held-back correction bits) as a lane-loop
    emulation: the scans glued by recode_progressive_finish == the original progressive JPEG == the host re-coder's output;
    truncated files are left to the host coder"""
    jpg, lep = golden(name)
    got, f = _progressive_scans_on_the_emulation(emu, jpg, lep)
    if "truncated" in name:
        assert got is None
        return
    assert got is not None, "eligible fixture was refused"
    assert f.recode() == jpg
    assert got == jpg


@pytest.mark.parametrize("name", [n for n in golden_cases() if n.startswith("prog_") and "truncated" not in n])
def test_lane_per_unit_progressive_scan_encoder_restores_the_jpeg(emu, name):
    """lep_huffprog_simt.h (count / place / assign / code / stuff, one lane per 32 blocks) as a lane-loop emulation: every scan
    byte-equal to the wavefront-per-scan form's, the glued file == the original; files with restart intervals stay with the
    wavefront form"""
    jpg, lep = golden(name)
    taken = []
    got, f = _progressive_scans_on_the_emulation(emu, jpg, lep, simt=True, taken_out=taken)
    assert got is not None and got == jpg
    assert all(taken) != ("rst" in name), taken


def _prog_plan_for(jpg, lep):
    """(file, image, scans, n) of an eligible progressive file: the descriptors lep_file_recode_plan_progressive fills"""
    from lepton_amd import abi
    from lepton_amd.codec import LepFile

    L = abi.lib()
    f = LepFile(lep)
    img = abi.HuffProgImage()
    scans = (abi.HuffProgScan * 64)()
    nscan, ok = C.c_int(0), C.c_int(0)
    assert L.lep_file_recode_plan_progressive(f.handle, C.byref(img), scans, 64, C.byref(nscan), C.byref(ok)) == 0
    assert ok.value
    return f, img, scans, nscan.value


def _both_scan_writers(emu, img, scans, n, region=0):
    """every scan of the plan through the wavefront form and the lane-per-unit form: [(bytes, bytes)]"""
    out_total = corr_total = 0
    for i in range(n):
        scans[i].image = 0
        scans[i].out_off = out_total
        out_total += (scans[i].out_cap + 15) & ~15
        scans[i].corr_off = corr_total
        corr_total += scans[i].corr_cap
    corr = (C.c_uint32 * (corr_total + 8))()
    outs, lens = [], []
    for form in (0, 1):
        out = C.create_string_buffer(out_total + 64)
        ln = (C.c_uint32 * n)()
        if form == 0:
            emu.emu_huffman_progressive_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
            assert emu.emu_huffman_progressive_encode(C.byref(img), scans, n, out, corr, ln) == 0
        else:
            taken = (C.c_int32 * n)()
            emu.emu_huffman_progressive_encode_simt.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
            assert emu.emu_huffman_progressive_encode_simt(C.byref(img), scans, n, out, corr, ln, taken, region) == 0
            assert all(taken)
        outs.append(out)
        lens.append(list(ln))
    return [(lens[0][i], outs[0].raw[scans[i].out_off: scans[i].out_off + (lens[0][i] & 0x7fffffff)],
             lens[1][i], outs[1].raw[scans[i].out_off: scans[i].out_off + (lens[1][i] & 0x7fffffff)]) for i in range(n)]


def test_lane_per_unit_progressive_scan_encoder_on_drawn_frames(emu):
    """the two forms on frames drawn as coefficients (not every one a frame a decoder could have produced -- the writers do not
    care): densities from empty to full, long stretches of blocks with nothing in a band (end-of-band runs across many units),
    tables whose longest run is 1 / 3 / 7 / 31 blocks (the run arithmetic modulo that), one block wide and one block high
    components"""
    import numpy as np
    from lepton_amd import corpus

    rng = np.random.default_rng(77)
    cases = 0
    for trial, (w, h, sub) in enumerate([(160, 120, "4:2:0"), (203, 149, "4:4:4"), (8, 600, "4:2:0"), (700, 8, "4:2:2"), (333, 241, "4:2:0"), (96, 64, "4:2:2")]):
        jpg = corpus.synth_jpeg(w, h, 600 + trial, progressive=True, subsampling=sub, quality=[90, 60, 95, 30, 75, 85][trial])
        img0 = JpegImage(jpg)
        streams, _ = ob.oracle_encode(img0.desc, img0.plan())
        f, img, scans, n = _prog_plan_for(jpg, img0.write_lep(streams))
        for variant in range(5):
            for c in range(f.desc.ncomp):
                nb = f.desc.nblocks(c)
                arr = np.zeros((nb, 64), dtype=np.int16)
                dens = [0.0, 0.02, 0.15, 0.6, 1.0][variant]
                mask = rng.random((nb, 64)) < dens
                vals = rng.integers(-40, 41, (nb, 64)).astype(np.int16)
                if variant == 3:
                    vals = rng.integers(-2000, 2001, (nb, 64)).astype(np.int16)
                arr[mask] = vals[mask]
                if variant in (1, 2):   # whole stretches of blocks with nothing in them, and blocks that only hold old coefficients
                    for _ in range(4):
                        a = int(rng.integers(0, nb)); b = min(nb, a + int(rng.integers(1, max(2, nb // 2))))
                        arr[a:b] = 0 if rng.random() < 0.5 else (arr[a:b] & ~1) * 2
                C.memmove(f.desc.blocks[c], arr.ctypes.data, nb * 128)
            for mx in (0, 1, 3, 7, 31):
                keep = [scans[i].max_eobrun for i in range(n)]
                if mx:
                    for i in range(n):
                        if scans[i].to != 0:
                            scans[i].max_eobrun = min(mx, keep[i])
                res = _both_scan_writers(emu, img, scans, n)
                outgrown = any(l0 & 0x80000000 for l0, _, _, _ in res) or sum(l0 for l0, _, _, _ in res) > len(jpg)
                for i, (l0, b0, l1, b1) in enumerate(res):
                    if l0 & 0x80000000:     # (a drawn frame may code to more than the file the plan was made for: both forms say so)
                        assert l1 & 0x80000000, (trial, variant, mx, i)
                        continue
                    if outgrown and (l1 & 0x80000000):   # (... and the scans behind it found the file's region used up)
                        continue
                    assert l0 == l1 and b0 == b1, (trial, variant, mx, i, scans[i].from_, scans[i].to, scans[i].sah, scans[i].sal, l0, l1)
                    cases += 1
                for i in range(n):
                    scans[i].max_eobrun = keep[i]
    assert cases > 500


def test_lane_per_unit_progressive_scan_encoder_on_runs_past_32767_blocks(emu):
    """a 2048 x 2048 frame whose bands are empty for tens of thousands of blocks in a row: an end-of-band run is written when it
    reaches 32767 blocks and the next begins (encode_eobrun, jpgcoder.cc:5337-5368); the lane-per-unit form finds those
    places by arithmetic"""
    import numpy as np
    from lepton_amd import corpus

    jpg = corpus.synth_jpeg(2048, 2048, 610, progressive=True, subsampling="4:4:4", quality=20)
    img0 = JpegImage(jpg)
    streams, _ = ob.oracle_encode(img0.desc, img0.plan())
    f, img, scans, n = _prog_plan_for(jpg, img0.write_lep(streams))
    assert any(scans[i].max_eobrun == 32767 for i in range(n))
    rng = np.random.default_rng(3)
    for c in range(f.desc.ncomp):
        nb = f.desc.nblocks(c)
        arr = np.zeros((nb, 64), dtype=np.int16)
        for at in ([5, 40000, 40001, 65000] if c == 0 else ([32767 + 3] if c == 1 else [])):
            arr[at] = rng.integers(-9, 10, 64)
        C.memmove(f.desc.blocks[c], arr.ctypes.data, nb * 128)
    for i, (l0, b0, l1, b1) in enumerate(_both_scan_writers(emu, img, scans, n)):
        assert l0 == l1 and b0 == b1, (i, l0, l1)


def test_lane_per_unit_progressive_scan_encoder_says_when_its_region_is_too_small(emu):
    """the bit buffers of a file's scans share a region sized by the file; when it does not suffice the scans left without one
    answer "outgrew" (bit 31) and the rest are still right"""
    from lepton_amd import corpus

    jpg = corpus.synth_jpeg(320, 240, 611, progressive=True)
    img0 = JpegImage(jpg)
    streams, _ = ob.oracle_encode(img0.desc, img0.plan())
    f, img, scans, n = _prog_plan_for(jpg, img0.write_lep(streams))
    src = JpegImage(jpg)
    for c in range(f.desc.ncomp):
        C.memmove(f.desc.blocks[c], src.desc.blocks[c], f.desc.nblocks(c) * 128)
    res = _both_scan_writers(emu, img, scans, n, region=len(jpg) // 2)
    assert any(l1 & 0x80000000 for _, _, l1, _ in res) and any(not (l1 & 0x80000000) for _, _, l1, _ in res)
    for l0, b0, l1, b1 in res:
        assert (l1 & 0x80000000) or (l0 == l1 and b0 == b1)


def test_gpu_progressive_scan_encoder_on_random_files(emu):
    """PIL-written progressive files over sizes, samplings, qualities and restart intervals (long end-of-band runs in smooth
    images, 4:4:4 / 4:2:2 / 4:2:0 / grey, non-multiple-of-MCU sizes): emulated GPU scans == the input JPEG"""
    import io
    import random

    import numpy as np
    from PIL import Image
    from lepton_amd import corpus
    from lepton_amd.codec import GpuCodec  # noqa: F401  (binding only)

    rnd = random.Random(5)
    done = 0
    for trial in range(14):
        w, h = rnd.choice([64, 97, 200, 333]), rnd.choice([48, 72, 150, 241])
        mode = rnd.choice(["RGB", "RGB", "L"])
        rng = np.random.default_rng(900 + trial)
        base = rng.integers(0, 256, (max(2, h // 24), max(2, w // 24), 3), dtype=np.uint8)
        a = np.asarray(Image.fromarray(base, "RGB").resize((w, h), Image.BICUBIC)).astype(np.int16)
        a = np.clip(a + rng.normal(0, rnd.choice([0, 2, 10, 40]), a.shape), 0, 255).astype(np.uint8)
        kw = dict(format="JPEG", quality=rnd.choice([30, 75, 92, 100]), progressive=True)
        if mode == "RGB":
            kw["subsampling"] = rnd.choice([0, 1, 2])
        if rnd.random() < 0.4:
            kw["restart_marker_blocks"] = rnd.choice([1, 3, 7])
        buf = io.BytesIO()
        Image.fromarray(a, "RGB").convert(mode).save(buf, **kw)
        jpg = buf.getvalue()
        img = JpegImage(jpg)
        streams, _ = ob.oracle_encode(img.desc, img.plan())
        lep = img.write_lep(streams)
        got, _ = _progressive_scans_on_the_emulation(emu, jpg, lep, simt=True)
        assert got is not None and got == jpg, (trial, w, h, mode, kw)
        done += 1
    assert done == 14


def _progressive_decode_on_the_emulation(emu, jpg, pipelined=False, deps_out=None, win=False, rows_out=None):
    """progressive scans of `jpg` through lep_huffprogdec.h (lane-loop emulation), level by level or as the one pipelined launch
    small batches take.  Returns (handle, frame planes, status): status None = not eligible, -1 = the kernels found it irregular,
    0 = decoded and finished.  win: through lep_huffprogdec_win.h (the window of speculative codes) where that form takes the scan;
    rows_out: receives every record the kernels wrote (bit positions, last DCs, pad bits | status)"""
    from lepton_amd import abi

    L = abi.lib()
    h = C.c_void_p()
    plan1 = abi.HuffDecImage()
    ok = C.c_int(0)
    rc = L.lep_jpeg_open_gpu(jpg, len(jpg), C.byref(h), C.byref(plan1), C.byref(ok))
    assert rc == 0 and not ok.value, "a progressive file is not the sequential kernel's"
    scans = (abi.HuffProgDecScan * 64)()
    nscan, need, ok2 = C.c_int(0), C.c_int(0), C.c_int(0)
    assert L.lep_jpeg_open_gpu_progressive(h, scans, 64, C.byref(nscan), C.byref(need), C.byref(ok2)) == 0
    if not ok2.value:
        L.lep_jpeg_close(h)
        return None, None, None
    d = abi.ImageDesc()
    L.lep_jpeg_describe(h, C.byref(d))
    planes = [C.create_string_buffer(d.nblocks(c) * 128) for c in range(d.ncomp)]
    p, n = C.c_void_p(), C.c_size_t(0)
    L.lep_jpeg_scan_bytes(h, C.byref(p), C.byref(n))
    raw = C.string_at(p, n.value)
    keep = []
    for i in range(nscan.value):
        off, ln = scans[i].t.scan or 0, scans[i].t.scan_len
        buf = C.create_string_buffer(raw[off:off + ln] + bytes(80), ln + 80)   # every scan in its own aligned, zero-padded slot
        keep.append(buf)
        scans[i].t.scan = C.addressof(buf)
        for c in range(d.ncomp):
            scans[i].t.blocks[c] = C.addressof(planes[c])
    rows = (abi.HuffDecRow * (need.value + 4))()
    if win:
        taken = C.c_int32(0)
        emu.emu_huffman_progressive_decode_win.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        assert emu.emu_huffman_progressive_decode_win(scans, nscan.value, rows, 1 if pipelined else 0, C.byref(taken)) == 0
        if deps_out is not None:
            deps_out.append(taken.value)
    elif pipelined:
        deps = (C.c_int32 * (4 * nscan.value))()
        emu.emu_huffman_progressive_decode_pipelined.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        assert emu.emu_huffman_progressive_decode_pipelined(scans, nscan.value, rows, deps) == 0
        if deps_out is not None:
            deps_out.extend([sorted(x for x in deps[4 * i: 4 * i + 4] if x >= 0), tuple(scans[i].cmp[k] for k in range(scans[i].cmpc)), scans[i].from_, scans[i].to, scans[i].sah]
                            for i in range(nscan.value))
    else:
        emu.emu_huffman_progressive_decode.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        assert emu.emu_huffman_progressive_decode(scans, nscan.value, rows) == 0
    if rows_out is not None:
        rows_out.extend((r.bitpos, tuple(r.last_dc), r.aux) for r in rows)
    rc = L.lep_jpeg_finish_gpu_progressive(h, scans, nscan.value, rows)
    return h, planes, (0 if rc == 0 else -1)


def _same_as_the_host_parser(jpg, h, planes):
    from lepton_amd import abi

    L = abi.lib()
    host = JpegImage(jpg)
    d = host.desc
    for c in range(d.ncomp):
        assert planes[c].raw == C.string_at(d.blocks[c], d.nblocks(c) * 128), "component %d differs" % c
    # hand-offs, pad bit, restart bookkeeping: the .lep header written from either handle must be the same bytes
    segs_h = (abi.Segment * abi.MAX_SEGMENTS)()
    n_h = L.lep_jpeg_plan(h, 8, segs_h, 0)
    segs = host.plan()
    assert n_h == len(segs) and all((segs_h[i].luma_y_start, segs_h[i].luma_y_end) == (segs[i].luma_y_start, segs[i].luma_y_end) for i in range(n_h))
    fake = [bytes([i + 1]) * 40 for i in range(n_h)]
    arr = (abi.Bytes * n_h)()
    bufs = []
    for i, s in enumerate(fake):
        b = C.create_string_buffer(s, len(s)); bufs.append(b)
        arr[i].data = C.cast(b, C.c_void_p).value; arr[i].len = arr[i].cap = len(s)
    out = abi.Bytes()
    assert L.lep_jpeg_write_lep(h, 8, arr, n_h, C.byref(out)) == 0
    got = out.tobytes(); L.lep_free(out.data)
    assert got == host.write_lep(fake), "container (hand-offs / pad bit / restart counts) differs from the host parser's"


SEQUENTIAL_SCAN_SCRIPTS = {            # (components: id, h, v, quantisation table, DC table, AC table; scans: component indices)
    "y_cbcr_420": ([(1, 2, 2, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)], [[0], [1, 2]]),
    "y_cb_cr_444": ([(1, 1, 1, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)], [[0], [1], [2]]),
    "ycb_cr_422": ([(1, 2, 1, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)], [[0, 1], [2]]),
    "cbcr_y_420": ([(1, 2, 2, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)], [[1, 2], [0]]),
    "cr_cb_y_440": ([(1, 1, 2, 0, 0, 0), (2, 1, 1, 1, 1, 1), (3, 1, 1, 1, 1, 1)], [[2], [1], [0]]),
    "y_cbcr_mixed": ([(1, 2, 2, 0, 0, 0), (2, 2, 1, 1, 1, 1), (3, 1, 2, 1, 1, 1)], [[0], [1, 2]]),
    "two_y_c": ([(1, 2, 1, 0, 0, 0), (2, 1, 1, 1, 1, 1)], [[0], [1]]),
}


@pytest.mark.parametrize("name", sorted(SEQUENTIAL_SCAN_SCRIPTS))
def test_sequential_frames_in_several_scans_on_the_scan_kernels(emu, name):
    """SEQUENTIAL frames coded in several scans (luma alone, then Cb + Cr together; a scan per component; any order): format 'X' like
    progressive files, decoded and written by the reference with its sequential block loop under the general scan walk.  Their scans
    come through the progressive descriptors (from 0 / to 63) and go to the SEQUENTIAL kernels, each scan an image of its own
    (VERDICT round 5 next #6): the scan decoders -- single wave, one lane per subsequence -- must leave the host parser's frame and a
    container that is the host parser's byte for byte (a hand-off record per MCU row of every scan of several components or of
    component 0, one per other scan); the scan encoders -- single wave, one lane per unit -- must write every scan as the host re-coder
    does.  Widths and heights with and without padding blocks, restart intervals (which count BLOCKS in a one-component scan)."""
    import jpeg_writer as jw
    import numpy as np
    import zlib
    from lepton_amd import abi

    L = abi.lib()
    comps, scans = SEQUENTIAL_SCAN_SCRIPTS[name]
    for w, h, ri, dens in [(97, 50, 0, 0.3), (96, 64, 5, 0.3), (640, 480, 0, 0.6), (333, 250, 7, 0.2), (8, 8, 0, 0.5), (17, 9, 1, 0.5), (1300, 40, 0, 0.02)]:
        jpg, _ = jw.write_sequential_scans(w, h, comps, np.random.default_rng(zlib.crc32(("%s %d %d" % (name, w, h)).encode())), scans, restart_interval=ri, density=dens)
        host = JpegImage(jpg)
        lep = host.write_lep(ob.oracle_encode(host.desc, host.plan())[0])
        assert lep[3:4] == b"X"
        for kw in (dict(), dict(pipelined=True), dict(win=True), dict(win=True, pipelined=True)):
            hnd, planes, status = _progressive_decode_on_the_emulation(emu, jpg, **kw)
            assert status == 0, (name, w, h, ri, kw, status)
            _same_as_the_host_parser(jpg, hnd, planes)
            L.lep_jpeg_close(hnd)
        for simt in (False, True):
            got, f = _progressive_scans_on_the_emulation(emu, jpg, lep, simt=simt)
            assert got is not None, (name, w, h, ri, "not planned for the GPU scan encoders")    # (a scan whose components use different tables too: "ycb_cr_422")
            assert got == jpg, (name, w, h, ri, simt)
        res = _progressive_check_on_the_emulation(emu, jpg)
        assert res is not None
        for length, got, want in res:
            assert length == len(want) and got == want


def test_sequential_scans_finish_refuses_a_chroma_record_behind_its_scan(emu):
    """lep_jpeg_finish_gpu_progressive on a sequential frame coded in several scans: the row records the scan decoders leave are accepted
    as they are; the same records with the first record of a one-component CHROMA scan pointing behind that scan's last bit -- what a
    stale record in the reused rows arena would look like -- are refused like every other record past its scan, not used as an index
    into the scan bytes."""
    import jpeg_writer as jw
    import numpy as np
    from lepton_amd import abi

    L = abi.lib()
    comps, script = SEQUENTIAL_SCAN_SCRIPTS["y_cb_cr_444"]
    jpg, _ = jw.write_sequential_scans(97, 50, comps, np.random.default_rng(20), script, density=0.3)
    valid = []
    hnd, planes, status = _progressive_decode_on_the_emulation(emu, jpg, rows_out=valid)
    assert status == 0                                   # the valid records, finished by the same entry point
    _same_as_the_host_parser(jpg, hnd, planes)
    L.lep_jpeg_close(hnd)

    def finish(patch):
        h, plan1, ok = C.c_void_p(), abi.HuffDecImage(), C.c_int(0)
        assert L.lep_jpeg_open_gpu(jpg, len(jpg), C.byref(h), C.byref(plan1), C.byref(ok)) == 0 and not ok.value
        scans = (abi.HuffProgDecScan * 64)()
        nscan, need, ok2 = C.c_int(0), C.c_int(0), C.c_int(0)
        assert L.lep_jpeg_open_gpu_progressive(h, scans, 64, C.byref(nscan), C.byref(need), C.byref(ok2)) == 0 and ok2.value and nscan.value == 3
        rows = (abi.HuffDecRow * len(valid))()
        for r, (bitpos, last_dc, aux) in zip(rows, valid):
            r.bitpos, r.aux = bitpos, aux
            for i in range(4):
                r.last_dc[i] = last_dc[i]
        chroma = [scans[i] for i in range(nscan.value) if scans[i].cmpc == 1 and scans[i].cmp[0] != 0]
        assert len(chroma) == 2
        patch(rows, chroma[0])
        rc = L.lep_jpeg_finish_gpu_progressive(h, scans, nscan.value, rows)
        L.lep_jpeg_close(h)
        return rc

    def at_the_end(rows, sc):
        rows[sc.t.rows_off].bitpos = sc.t.scan_len * 8            # the last position a record may name

    def past_the_end(rows, sc):
        rows[sc.t.rows_off].bitpos = sc.t.scan_len * 8 + 1

    assert finish(lambda rows, sc: None) == 0
    assert finish(at_the_end) == 0
    assert finish(past_the_end) != 0


def test_restart_interval_that_changes_from_scan_to_scan(emu):
    """A DRI segment may stand in front of ANY scan: the progressive files of phone cameras (the reference's images/androidprogressive.jpg,
    iphoneprogressive2.jpg) set one per scan -- 258 / 516, 768 / 1524 MCUs or blocks, a row of the scan's own units.  Until the end of round 6
    both scan plans sent such files to the host; every descriptor carries its own interval now (lep_huffprogdec_scan.t.rsti,
    lep_huffprog_scan.rsti).  The two reference images and sequential frames in several scans with an interval per scan (0 among them), both
    directions, every form of the kernels."""
    import jpeg_writer as jw
    import numpy as np
    import zlib
    from conftest import ref_golden, REF_GOLDEN
    from lepton_amd import abi

    L = abi.lib()
    files = []
    if os.path.exists(os.path.join(REF_GOLDEN, "androidprogressive.jpg")):
        files += [("ref:" + n,) + ref_golden(n) for n in ("androidprogressive", "iphoneprogressive2")]
    for name, intervals in [("y_cbcr_420", [12, 5]), ("y_cb_cr_444", [0, 7, 3]), ("cbcr_y_420", [4, 0]), ("two_y_c", [1, 40])]:
        comps, scans = SEQUENTIAL_SCAN_SCRIPTS[name]
        for w, h in [(97, 50), (333, 250)]:
            jpg, _ = jw.write_sequential_scans(w, h, comps, np.random.default_rng(zlib.crc32(("dri %s %d" % (name, w)).encode())), scans, restart_intervals=intervals, density=0.3)
            host = JpegImage(jpg)
            files.append(("%s %dx%d %s" % (name, w, h, intervals), jpg, host.write_lep(ob.oracle_encode(host.desc, host.plan())[0])))
    assert len(files) >= 8
    for name, jpg, lep in files:
        for kw in (dict(), dict(pipelined=True), dict(win=True, pipelined=True)):
            hnd, planes, status = _progressive_decode_on_the_emulation(emu, jpg, **kw)
            assert status == 0, (name, kw, status)
            _same_as_the_host_parser(jpg, hnd, planes)
            L.lep_jpeg_close(hnd)
        for simt in (False, True):
            got, f = _progressive_scans_on_the_emulation(emu, jpg, lep, simt=simt)
            assert got is not None and got == jpg, (name, simt)
        res = _progressive_check_on_the_emulation(emu, jpg)
        assert res is not None and all(length == len(want) and got == want for length, got, want in res), name


def test_progressive_scans_follow_the_right_scans(emu):
    """lep_huffprogdec.h prog_scan_deps: in the one pipelined launch a scan waits for exactly the scans of its file whose
    coefficients it reads or overwrites -- same component, bands that meet, earlier in the file -- minus those another of them
    already waits for.  libjpeg's default script (ten scans): the luma refinement follows BOTH first-stage luma scans, the last
    luma scan follows only the refinement in front of it, the DC refinement follows the DC scan, chroma follows chroma"""
    from lepton_amd import abi, corpus

    jpg = corpus.synth_jpeg(160, 120, 3, progressive=True)
    deps = []
    h, planes, st = _progressive_decode_on_the_emulation(emu, jpg, pipelined=True, deps_out=deps)
    assert st == 0
    _same_as_the_host_parser(jpg, h, planes)
    abi.lib().lep_jpeg_close(h)
    assert len(deps) == 10
    follows = [d[0] for d in deps]
    assert follows[:5] == [[], [], [], [], []]                  # first-stage scans: the frame starts zeroed
    for j, (dj, cmpj, fj, tj, sahj) in enumerate(deps):          # the general rule, checked against a direct statement of it
        want = [i for i in range(j) if set(deps[i][1]) & set(cmpj) and not (deps[i][2] > tj or fj > deps[i][3])]
        want = [i for i in want if not any(i < k and set(deps[i][1]) & set(deps[k][1]) and not (deps[i][2] > deps[k][3] or deps[k][2] > deps[i][3]) for k in want)]
        assert dj == want, (j, dj, want)
    assert follows[5] == [1, 4] and follows[6] == [0] and follows[9] == [5]


@pytest.mark.parametrize("pipelined", [False, True], ids=["level_by_level", "one_pipelined_launch"])
@pytest.mark.parametrize("name", [n for n in golden_cases() if n.startswith("prog_")])
def test_gpu_progressive_scan_decoder_on_cpu_equals_the_host_parser(emu, name, pipelined):
    """lep_huffprogdec.h (DC / AC first-stage and refinement scans, end-of-band runs, correction bits, dependency levels) as a
    lane-loop emulation: the frame and the .lep header equal the host parser's; truncated files are left to the host"""
    from lepton_amd import abi

    jpg, _ = golden(name)
    h, planes, st = _progressive_decode_on_the_emulation(emu, jpg, pipelined=pipelined)
    if "truncated" in name:
        assert st is None
        return
    assert st == 0, "eligible fixture was refused or found irregular"
    _same_as_the_host_parser(jpg, h, planes)
    abi.lib().lep_jpeg_close(h)


@pytest.mark.parametrize("pipelined", [False, True], ids=["level_by_level", "one_pipelined_launch"])
@pytest.mark.parametrize("name", [n for n in golden_cases() if n.startswith("prog_") and "truncated" not in n])
def test_window_progressive_scan_decoder_on_cpu_equals_the_host_parser(emu, name, pipelined):
    """lep_huffprogdec_win.h (every lane decodes the code that would start at its bit, the chain hops between them on the scalar
    unit; correction bits fetched by their lanes) as a lane-loop emulation: the frame and the .lep header equal the host
    parser's, the records equal lep_huffprogdec.h's; the fixture with restart intervals stays with that form"""
    from lepton_amd import abi

    jpg, _ = golden(name)
    taken, rows_w, rows_o = [], [], []
    h, planes, st = _progressive_decode_on_the_emulation(emu, jpg, pipelined=pipelined, win=True, deps_out=taken, rows_out=rows_w)
    assert st == 0, "eligible fixture was refused or found irregular"
    assert (taken[0] > 0) != ("rst" in name)
    _same_as_the_host_parser(jpg, h, planes)
    abi.lib().lep_jpeg_close(h)
    h2, planes2, st2 = _progressive_decode_on_the_emulation(emu, jpg, pipelined=pipelined, rows_out=rows_o)
    abi.lib().lep_jpeg_close(h2)
    assert st2 == 0 and rows_w == rows_o


def _mutated_progressive(rnd, seeds):
    j = bytearray(rnd.choice(seeds))
    sos = j.find(b"\xff\xda")
    k = rnd.choice(["flip", "byte", "del", "ins", "hdr", "flip", "byte"])
    pos = rnd.randrange(sos, len(j) - 2) if k != "hdr" else rnd.randrange(2, sos)
    if k == "flip":
        j[pos] ^= 1 << rnd.randrange(8)
    elif k == "byte":
        j[pos] = rnd.randrange(256)
    elif k == "del":
        del j[pos:pos + rnd.choice([1, 2, 5])]
    elif k == "ins":
        j[pos:pos] = bytes(rnd.randrange(256) for _ in range(rnd.choice([1, 2])))
    else:
        j[pos] ^= 1 << rnd.randrange(8)
    return bytes(j), k


def test_window_progressive_scan_decoder_on_damaged_files(emu):
    """progressive files damaged inside their scans (bit flips, overwritten / deleted / inserted bytes) and in their headers:
    the window form refuses exactly the files the uniform-code form refuses, and where both decode, frame and records are the
    same -- so the host parser is asked for the same files as before"""
    import random
    from lepton_amd import abi

    rnd = random.Random(61)
    seeds = [golden(n)[0] for n in golden_cases() if n.startswith("prog_") and "trunc" not in n and "rst" not in n and len(golden(n)[0]) < 30000]
    both = refused = 0
    for trial in range(220):
        j, kind = _mutated_progressive(rnd, seeds)
        res = []
        for win in (False, True):
            rows = []
            try:
                h, planes, st = _progressive_decode_on_the_emulation(emu, j, pipelined=bool(trial & 1), win=win, rows_out=rows)
            except AssertionError:
                res.append(None)      # not openable / not a progressive file any more: neither form is asked
                continue
            if st is not None:
                abi.lib().lep_jpeg_close(h)
            res.append((st, [p.raw for p in planes] if st == 0 else None, [r[2] >> 8 for r in rows] if st is not None else None, rows if st == 0 else None))
        if res[0] is None or res[1] is None:
            assert res[0] is None and res[1] is None, (trial, kind)
            continue
        assert res[0][0] == res[1][0], (trial, kind, res[0][0], res[1][0])
        if res[0][0] == 0:
            assert res[0][1] == res[1][1] and res[0][3] == res[1][3], (trial, kind)
            both += 1
        elif res[0][0] == -1:
            refused += 1
    assert both >= 20 and refused >= 60, (both, refused)


def test_gpu_progressive_scan_decoder_on_random_files(emu):
    import io
    import random

    import numpy as np
    from PIL import Image
    from lepton_amd import abi

    rnd = random.Random(6)
    done = 0
    for trial in range(16):
        w, h_ = rnd.choice([64, 97, 200, 333]), rnd.choice([48, 72, 150, 241])
        mode = rnd.choice(["RGB", "RGB", "L"])
        rng = np.random.default_rng(700 + trial)
        base = rng.integers(0, 256, (max(2, h_ // 24), max(2, w // 24), 3), dtype=np.uint8)
        a = np.asarray(Image.fromarray(base, "RGB").resize((w, h_), Image.BICUBIC)).astype(np.int16)
        a = np.clip(a + rng.normal(0, rnd.choice([0, 2, 10, 40]), a.shape), 0, 255).astype(np.uint8)
        kw = dict(format="JPEG", quality=rnd.choice([30, 75, 92, 100]), progressive=True)
        if mode == "RGB":
            kw["subsampling"] = rnd.choice([0, 1, 2])
        if rnd.random() < 0.4:
            kw["restart_marker_blocks"] = rnd.choice([1, 3, 7])
        buf = io.BytesIO()
        Image.fromarray(a, "RGB").convert(mode).save(buf, **kw)
        jpg = buf.getvalue()
        for win in (False, True):    # lep_huffprogdec.h, then lep_huffprogdec_win.h (files with restart intervals: the former both times)
            hdl, planes, st = _progressive_decode_on_the_emulation(emu, jpg, pipelined=trial % 2 == 1, win=win)   # level by level / one pipelined launch, in turn
            assert st == 0, (trial, w, h_, mode, kw, st, win)
            _same_as_the_host_parser(jpg, hdl, planes)
            abi.lib().lep_jpeg_close(hdl)
        done += 1
    assert done == 16


def _emulated_gpu_scan_encode(emu, f):
    """plan -> lep_huff.h (lep_huff_simt.h for a file cut inside its scan) as a lane loop per segment -> finish; None when the file is not
    eligible for the GPU scan encoder or the encoder leaves it to the host re-coder"""
    from lepton_amd import abi
    L = abi.lib()
    img = abi.HuffImage()
    segs = (abi.HuffSegment * abi.MAX_SEGMENTS)()
    nseg, ok = C.c_int(0), C.c_int(0)
    assert L.lep_file_recode_plan(f.handle, C.byref(img), segs, C.byref(nseg), C.byref(ok)) == 0
    if not ok.value:
        return None
    outs = (abi.Bytes * nseg.value)()
    ends = (abi.HuffEnd * nseg.value)()
    keep = []
    for i in range(nseg.value):
        cap = min(segs[i].out_cap, 1 << 24)
        segs[i].out_cap = cap
        buf = C.create_string_buffer(cap + 8)
        keep.append(buf)
        n = C.c_uint32(0)
        # lep_gpu_huffman_encode_device's routing: the lane-per-unit kernels take what they can (restart intervals included), the
        # wavefront-per-segment kernel the rest -- except a file cut inside its scan, which is the lane-per-unit kernels' or nobody's, and
        # the host re-coder's whenever the cut is met before the byte bound (LEP_GPU_PATH_DECLINED, what the batch decompressor acts on)
        if emu.emu_huffman_encode_segment_simt(C.byref(img), C.byref(segs[i]), buf, C.byref(n), C.byref(ends[i])) != 0:
            if any(img.trunc_bc[c] for c in range(4)):
                return None
            assert emu.emu_huffman_encode_segment(C.byref(img), C.byref(segs[i]), buf, C.byref(n), C.byref(ends[i])) == 0
        outs[i].data = C.cast(buf, C.c_void_p).value
        outs[i].len = outs[i].cap = n.value
    out = abi.Bytes()
    rc = L.lep_file_recode_finish(f.handle, outs, ends, nseg.value, C.byref(out))
    if rc == 101:
        return None
    assert rc == 0, rc
    got = out.tobytes()
    L.lep_free(out.data)
    return got


def test_gpu_scan_encoder_on_cpu_restores_the_format_2_fixtures(emu):
    """the files of tests/golden/v2 (brotli headers, every segment bound by its size, chained and merged streams, the
    reference's own narrowrst.lep) through the GPU path's host halves around the emulated scan encoder: same bytes as the
    host re-coder, which test_format_v2 holds against the reference -- the segment byte counts recode_finish checks against
    the hand-offs (recoder.cc:625-640) are those of intact files"""
    import json
    import os
    import oracle_binding as ob
    from conftest import GOLDEN
    from lepton_amd.codec import lep_stream

    v2 = os.path.join(GOLDEN, "v2")
    ran = 0
    for name in sorted(json.load(open(os.path.join(v2, "manifest.json")))):
        for f in lep_stream(open(os.path.join(v2, name + ".lep"), "rb").read()):
            ob.oracle_decode(f.desc, f.segments, f.streams)
            want = f.recode()
            got = _emulated_gpu_scan_encode(emu, f)
            if got is not None:
                assert got == want, name
                ran += 1
    assert ran >= 8


def test_gpu_scan_encoder_on_cpu_gives_the_reference_s_answers_for_damaged_hand_offs(emu):
    """the hand-off field mutants of tests/test_fuzz_host.py (each pinned to what the reference binary answers) through the GPU
    path's host halves around the emulated scan encoder: plan (which sends what the kernel cannot reproduce to the host
    re-coder: bit counts of 8 and more, pre-hand-off records, bounds that wrap or leave room for nothing), lane-loop kernel,
    finish -- the same bytes, or the file is not eligible and the host re-coder is what runs on the GPU box too"""
    import hashlib
    import oracle_binding as ob
    from lepton_amd.codec import LepFile, LeptonError
    from test_fuzz_host import hand_off_field_cases

    through_the_kernel = 0
    for i, (lep, want) in enumerate(hand_off_field_cases()):
        try:
            f = LepFile(lep)
        except LeptonError as e:
            assert e.code == want, i
            continue
        ob.oracle_decode(f.desc, f.segments, f.streams)
        try:
            got = _emulated_gpu_scan_encode(emu, f)
        except AssertionError as e:          # lep_file_recode_finish refused: its code is the assertion's message
            got = int(str(e).split()[0])
        if got is None:
            continue
        through_the_kernel += 1
        assert (got if isinstance(got, int) else (len(got), hashlib.md5(got).hexdigest())) == want, i
    assert through_the_kernel >= 3


def test_v4_decoder_on_a_first_segment_that_starts_inside_the_image(emu):
    """a damaged hand-off can make the FIRST segment start at an MCU row other than 0 (lep_file_segments rounds a luma_y_start
    inside an MCU row up, as the reference's baseline re-coder does): the decoder kernel treats that row as a top row, like any
    later segment's first row -- frames equal the oracle's.  The second case is the truncated fixture, where the shift turns the
    stream into garbage: edges that claim more non-zeros than positions are left.  Round 2's edge round read a neighbouring
    pair's Branch there; it now indexes like the reference (decoder.cc:58-141) and the frame is the oracle's."""
    import oracle_binding as ob
    from lepton_amd.codec import LepFile
    from test_fuzz_host import hand_off_field_cases

    for lep, _ in hand_off_field_cases()[:2]:
        f = LepFile(lep)
        d, segs = f.desc, f.segments
        assert len(segs) == 1 and segs[0].luma_y_start > 0
        ob.oracle_decode(d, segs, f.streams)
        want = [C.string_at(d.blocks[c], d.nblocks(c) * 128) for c in range(d.ncomp)]
        for c in range(d.ncomp):
            C.memset(d.blocks[c], 0, d.nblocks(c) * 128)
        s, wv = segs[0], f.streams[0]
        for gen in ("v4",):
            for c in range(d.ncomp):
                C.memset(d.blocks[c], 0, d.nblocks(c) * 128)
            assert getattr(emu, "emu_decode_segment_" + gen)(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, wv, len(wv), None) == 0
            assert [C.string_at(d.blocks[c], d.nblocks(c) * 128) for c in range(d.ncomp)] == want


@pytest.fixture
def edge_count_bias():
    """oracle knob: its encoder claims 2 more edge non-zeros than a block holds (oracle/lepton_oracle.c)"""
    L = ob.oracle()
    knob = C.c_int.in_dll(L, "lor_test_edge_count_bias")
    knob.value = 2
    yield knob
    knob.value = 0


@pytest.mark.parametrize("gen", ["", "_v4"])
@pytest.mark.parametrize("name", ["c420_odd_203x149", "gray_120x88", "c444_96x80", "truncated"])
def test_decoders_follow_the_reference_on_impossible_edge_counts(emu, edge_count_bias, name, gen):
    """a stream that claims more edge non-zeros than positions remain.  The reference indexes
    exponent_counts_x_ directly with the claimed count (decoder.cc:58-141) and decodes on; every kernel generation must read
    the same Branches (the v4 edge round holds one lane per REACHABLE (position, non-zeros-left) pair and takes a direct path
    for the others).  Expected frame: the original -- the biased encoder codes the true coefficients under the false count."""
    jpg, _ = golden(name)
    img = JpegImage(jpg)
    d = img.desc
    segs = img.plan()
    want, bins = ob.oracle_encode(d, segs)          # streams with impossible counts
    edge_count_bias.value = 0
    honest, _ = ob.oracle_encode(d, segs)
    assert want != honest
    orig = [C.string_at(d.blocks[c], d.nblocks(c) * 128) for c in range(d.ncomp)]
    ob.oracle_decode(d, segs, want)                 # the oracle (== reference decoder) restores the frame from them
    assert [C.string_at(d.blocks[c], d.nblocks(c) * 128) for c in range(d.ncomp)] == orig
    for c in range(d.ncomp):
        C.memset(d.blocks[c], 0, d.nblocks(c) * 128)
    for s, w in zip(segs, want):
        assert getattr(emu, "emu_decode_segment" + gen)(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, w, len(w), None) == 0
    for c in range(d.ncomp):
        n = d.coded_blocks[c] * 128
        assert C.string_at(d.blocks[c], n) == orig[c][:n]


def test_v4_other_forms_on_impossible_edge_counts(emu_other_forms, edge_count_bias):
    """the same with the edge round's serial code on the scalar unit (LEP_DEC4_SCALAR=13)"""
    jpg, _ = golden("c420_odd_203x149")
    img = JpegImage(jpg)
    d = img.desc
    segs = img.plan()
    want, _ = ob.oracle_encode(d, segs)
    orig = [C.string_at(d.blocks[c], d.nblocks(c) * 128) for c in range(d.ncomp)]
    for c in range(d.ncomp):
        C.memset(d.blocks[c], 0, d.nblocks(c) * 128)
    for gen in ("v4",):
        for c in range(d.ncomp):
            C.memset(d.blocks[c], 0, d.nblocks(c) * 128)
        for s, w in zip(segs, want):
            assert getattr(emu_other_forms, "emu_decode_segment_" + gen)(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, w, len(w), None) == 0
        for c in range(d.ncomp):
            n = d.coded_blocks[c] * 128
            assert C.string_at(d.blocks[c], n) == orig[c][:n]


def test_gpu_scan_encoder_end_states_are_held_against_the_hand_offs(emu):
    """recode.cc:625-640 on the GPU path (missing #5): the scan encoder hands back the partial byte, its bit
    count and the last DCs every segment ends in; lep_file_recode_finish refuses a file where they are not what the next
    hand-off recorded -- all three, not only the byte count"""
    from lepton_amd import abi
    from lepton_amd.codec import LepFile

    jpg, lep = golden("q30_256x256_4seg")
    L = abi.lib()

    def run(mutate):
        f = LepFile(lep)
        ob.oracle_decode(f.desc, f.segments, f.streams)
        img = abi.HuffImage()
        segs = (abi.HuffSegment * abi.MAX_SEGMENTS)()
        nseg, ok = C.c_int(0), C.c_int(0)
        assert L.lep_file_recode_plan(f.handle, C.byref(img), segs, C.byref(nseg), C.byref(ok)) == 0 and ok.value and nseg.value >= 2
        N = nseg.value
        outs = (abi.Bytes * N)()
        ends = (abi.HuffEnd * N)()
        keep = []
        for i in range(N):
            buf = C.create_string_buffer(segs[i].out_cap + 8)
            keep.append(buf)
            n = C.c_uint32(0)
            assert emu.emu_huffman_encode_segment(C.byref(img), C.byref(segs[i]), buf, C.byref(n), C.byref(ends[i])) == 0
            outs[i].data = C.cast(buf, C.c_void_p).value
            outs[i].len = outs[i].cap = n.value
        states = [(e.overhang_byte, e.num_overhang_bits, tuple(e.last_dc)[:3], e.attempted) for e in ends]
        mutate(ends)
        out = abi.Bytes()
        rc = L.lep_file_recode_finish(f.handle, outs, ends, N, C.byref(out))
        got = out.tobytes() if rc == 0 else None
        if rc == 0:
            L.lep_free(out.data)
        return rc, got, states, f

    rc, got, states, f = run(lambda e: None)
    assert rc == 0 and got == jpg
    # what the kernel hands back IS what the file's hand-offs recorded
    src = JpegImage(jpg)
    hs = (abi.Handoff * abi.MAX_SEGMENTS)()
    N = L.lep_jpeg_plan_handoffs(src.handle, 0, hs, abi.MAX_SEGMENTS)
    assert N == len(states) >= 2
    for q in range(N - 1):
        assert states[q][:3] == (hs[q + 1].overhang_byte, hs[q + 1].num_overhang_bits, tuple(hs[q + 1].last_dc)[:3])
        assert states[q][3] == hs[q].segment_size

    def dc(e):
        e[N - 2].last_dc[2] += 1
    def bits(e):
        e[0].num_overhang_bits ^= 1
    def byte(e):
        e[0].overhang_byte ^= 0x80
    for m in (dc, bits, byte):
        assert run(m)[0] == 1          # ASSERTION_FAILURE, as recode_physical_thread answers
    def last(e):                        # the last segment's end state is held against nothing
        e[N - 1].last_dc[0] += 5
    assert run(last)[0] == 0


V5_ENTRIES = ("emu_encode_segment_v5", "emu_encode_segment_v5_halves", "emu_encode_segment_v5_parts")   # one wavefront per segment; the walks' two halves apart; gather and write in parts


def _v5_encode(emu, d, s, cap, entry="emu_encode_segment_v5"):
    buf = C.create_string_buffer(cap)
    n, nb = C.c_uint32(0), C.c_uint32(0)
    rc = getattr(emu, entry)(C.byref(d), s.luma_y_start, s.luma_y_end, s.is_last, buf, cap, C.byref(n), C.byref(nb), None, 0)
    return rc, buf.raw[: n.value], nb.value


@pytest.mark.parametrize("entry", V5_ENTRIES)
@pytest.mark.parametrize("name", golden_cases())
def test_split_phase_encoder_on_cpu_matches_oracle(emu, name, entry):
    """lep_enc5.h -- count / emit / fold per chain / gather / lane-per-segment writer -- stepped on the CPU: every segment's
    stream == the oracle's, and the bin list has the oracle's number of bins (minus the start marker and the 32 stop bins).
    `_halves`: the walks run as the two halves (7x7 interiors | records, edges, DC) two wavefronts share on the GPU"""
    jpg, _ = golden(name)
    img = JpegImage(jpg)
    d = img.desc
    segs = img.plan()
    want, bins = ob.oracle_encode(d, segs)
    total = 0
    for s, w in zip(segs, want):
        rc, got, nb = _v5_encode(emu, d, s, len(w) + 4096, entry)
        assert rc == 0
        assert got == w
        total += nb
    assert total == bins


@pytest.mark.parametrize("entry", V5_ENTRIES)
def test_split_phase_encoder_large_coefficients_and_refusals(emu, entry):
    """lep_enc5.h on blocks full of large coefficients (entries of several units, threshold units, exponent rows to the end) and
    the refusals in the serial coder's order: the FIRST offence in stream order names the exit code -- an out-of-range interior
    coefficient (6), a DC that does not survive prediction (6) in a block BEHIND it, an edge whose prior divides by zero (43)"""
    import numpy as np
    from lepton_amd import corpus

    img = JpegImage(corpus.synth_jpeg(64, 48, 11, quality=100))
    d = img.desc
    rng = np.random.default_rng(5)
    for c in range(d.ncomp):
        n = d.nblocks(c) * 64
        arr = (C.c_int16 * n).from_address(d.blocks[c])
        vals = rng.integers(-255, 256, n)
        vals[rng.random(n) < 0.1] = 0
        big = rng.random(n) < 0.004
        vals[big] = rng.choice([-2047, 2047, 1024, -1500], int(big.sum()))
        for i in range(n):
            arr[i] = int(vals[i])
        for b in range(d.nblocks(c)):
            arr[b * 64 + 49] = 0
    segs = img.plan()
    want, bins = ob.oracle_encode(d, segs)
    total = 0
    for s, w in zip(segs, want):
        rc, got, nb = _v5_encode(emu, d, s, len(w) + 4096, entry)
        assert rc == 0 and got == w
        total += nb
    assert total == bins
    # refusals: whatever the oracle answers, the split-phase encoder answers
    s = segs[0]

    def both():
        try:
            ob.oracle_encode(d, [s])
            o = 0
        except RuntimeError as e:
            o = int(str(e).rsplit(" ", 1)[1])
        return o, _v5_encode(emu, d, s, 1 << 20, entry)[0]

    luma = C.cast(d.blocks[0], C.POINTER(C.c_int16))
    chroma = C.cast(d.blocks[1], C.POINTER(C.c_int16))
    save = luma[64 * 3 + 5]
    luma[64 * 3 + 5] = 4096                       # interior coefficient of luma block 3: bit length 13
    assert both() == (6, 6)
    luma[64 * 3 + 5] = save
    save = chroma[49]
    chroma[49] = 3000                             # a DC the prediction cannot wrap back (first coded block of the segment)
    assert both() == (6, 6)
    chroma[49] = save
    assert both() == (0, 0)
    # an interior refusal in a block BEHIND a block whose DC is refused: the DC's block comes first in the stream
    s1, s2 = luma[64 * 5 + 5], luma[64 * 2 + 49]
    luma[64 * 5 + 5], luma[64 * 2 + 49] = 4096, 3000
    assert both() == (6, 6)
    luma[64 * 5 + 5], luma[64 * 2 + 49] = s1, s2
    assert both() == (0, 0)


def test_deferred_bool_writer_equals_the_serial_one(emu):
    """lep5::BoolEnc5 -- the lane-per-segment writer's deferred byte output and carry cache -- writes the bytes of
    lepdev::BoolCoder<false> (boolwriter.hh:48-118) for 12,000 random and adversarial bin sequences, overflow verdicts included"""
    assert emu.emu_check_bool_writer5(12000) == 0


def test_stitched_bool_writer_equals_the_serial_one(emu):
    """the stitched writer (lep_enc5.h: range / link / code / stitch -- a stream coded as K chunks whose start ranges are guessed from
    a warm-up, whose bit offsets come out of a scan over the chunks, and whose bytes are added together with their carries) writes the
    bytes of lepdev::BoolCoder<false> for 4,000 bin lists (to 40,000 bins, K = 2..64, warm-ups from 8 bins -- where nearly every guess
    is wrong and the link pass redoes the chunk -- to longer than the list), overflow verdicts included"""
    redone = C.c_int(0)
    assert emu.emu_check_stitched_writer5(4000, C.byref(redone)) == 0
    assert redone.value > 1000      # the wrong-guess path was walked


def test_sixteen_bit_branch_equals_the_packed_word(emu):
    """the fold lanes keep a Branch as two counts (lep5::upd16 / prob16, the saturated-true state as t = 0): same probabilities
    as lepdev::branch_update (branch.hh:82-100) along 900 random walks of every bias, saturation and renormalisation included"""
    assert emu.emu_check_branch16(900) == 0


def test_progressive_scan_dependencies_on_made_up_scripts(emu):
    """prog_scan_deps (lep_huffprogdec.h) on scan scripts libjpeg does not write: bands that overlap in part, DC refinement per
    component behind an interleaved DC scan, two files whose scans alternate in the launch, a scan behind five independent ones
    (no pipelining then), and a launch order that would make a scan wait for one behind it (refused)"""
    from lepton_amd import abi

    def run(rows, order=None):
        n = len(rows)
        scans = (abi.HuffProgDecScan * n)()
        for i, (frame, comps, lo, hi) in enumerate(rows):
            scans[i].t.blocks[0] = frame
            scans[i].cmpc = len(comps)
            for k, c in enumerate(comps):
                scans[i].cmp[k] = c
            scans[i].from_, scans[i].to = lo, hi
        od = (C.c_int * n)(*(order or range(n)))
        deps = (C.c_int32 * (4 * n))()
        emu.emu_prog_scan_deps.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        ok = emu.emu_prog_scan_deps(scans, od, n, deps)
        return ok, [sorted(x for x in deps[4 * i: 4 * i + 4] if x >= 0) for i in range(n)]

    A, B = 0x1000, 0x2000
    # bands that meet in part: 3..10 follows 1..5; 11..63 follows nothing; 1..63 refinement follows all three directly
    ok, d = run([(A, [0], 1, 5), (A, [0], 3, 10), (A, [0], 11, 63), (A, [0], 1, 63)])
    assert ok and d == [[], [0], [], [1, 2]]          # (0 is implied through 1)
    # interleaved DC, then DC refinement component by component; chroma AC scans follow nothing
    ok, d = run([(A, [0, 1, 2], 0, 0), (A, [1], 0, 0), (A, [0], 0, 0), (A, [2], 1, 63), (A, [2], 0, 0)])
    assert ok and d == [[], [0], [0], [], [0]]
    # two files in one launch, scans alternating: a scan never follows the other file's
    ok, d = run([(A, [0], 1, 63), (B, [0], 1, 63), (A, [0], 1, 63), (B, [0], 1, 63), (B, [0], 1, 63)], order=[0, 0, 1, 1, 2])
    assert ok and d == [[], [], [0], [1], [3]]
    # five independent bands in front of one scan that covers them all: more than four to wait for
    ok, _ = run([(A, [0], 1, 2), (A, [0], 3, 4), (A, [0], 5, 6), (A, [0], 7, 8), (A, [0], 9, 10), (A, [0], 1, 63)])
    assert not ok
    # the scan that comes first in the FILE stands behind the one that follows it in the LAUNCH: a wait that could never end
    ok, _ = run([(A, [0], 1, 63), (A, [0], 1, 63)], order=[1, 0])
    assert not ok


def _cut_jpegs():
    """files that end inside their scan (no EOI): [(name, bytes)] -- the truncated goldens, the reference's own truncated photographs, the
    file `lepton -benchmark` codes, and a 4:2:0 file cut at many places (in the first MCU row, at a row boundary, in the last bytes)"""
    import bench
    from conftest import ref_golden
    out = [(n, golden(n)[0]) for n in ("truncated", "truncated_short")]
    out += [(n, ref_golden(n)[0]) for n in ("truncatedzerorun", "singlerowtrunc")]
    out.append(("reference_benchmark_file", bench.reference_benchmark_jpeg()))
    whole = golden("c420_odd_203x149")[0]
    sos = whole.find(b"\xff\xda")
    for cut in (sos + 30, sos + 200, len(whole) // 2, len(whole) * 3 // 4, len(whole) - 40, len(whole) - 3, len(whole) - 2):
        out.append(("c420_odd_cut_at_%d" % cut, whole[:cut]))
    big = golden("q30_256x256_4seg")[0]      # several thread segments
    out += [("q97_4seg_cut_at_%d" % c, big[:c]) for c in (len(big) // 3, len(big) - 1000)]
    return out


@pytest.mark.parametrize("bits", [1024, 8192])
@pytest.mark.parametrize("name", [n for n, _ in _cut_jpegs()])
def test_lane_per_subsequence_huffman_decoder_on_files_cut_inside_their_scan(emu, name, bits):
    """A file without EOI ends inside its scan: the reference decodes up to the block that reads the data's last bit (zeros behind it) and
    codes what it has (uncompressed_components.hh:166-185).  lep_huffdec_simt.h + parse_jpeg_finish_gpu must leave exactly the host
    parser's frame, hand-offs and truncation bounds -- the .lep written from them is the host parser's (== the reference's for the
    fixtures) -- or report a status and leave the file to the host parser; never a different result."""
    jpg = dict(_cut_jpegs())[name]
    res = _cut_file_through_the_lane_per_subsequence_decoder(emu, jpg, bits)
    if isinstance(res, str):   # the kernels left the file to the host parser: its path is the product's
        _host_path(jpg, _golden_lep(name))


def _cut_file_through_the_lane_per_subsequence_decoder(emu, jpg, bits, stale=None):
    """the body of the test above: True when the kernels' answer was taken and is the host parser's, a string when it was not asked
    for or left the file to the host parser.  stale: a (bitpos, aux) record standing where the image's final record goes -- the
    record array is reused between launches"""
    from lepton_amd import abi

    L = abi.lib()
    try:
        host = JpegImage(jpg)
    except Exception:
        return "the host parser refuses this cut"
    h = C.c_void_p()
    img = abi.HuffDecImage()
    ok = C.c_int(0)
    assert L.lep_jpeg_open_gpu(jpg, len(jpg), C.byref(h), C.byref(img), C.byref(ok)) == 0
    if not ok.value:
        L.lep_jpeg_close(h)
        return "not eligible for the GPU scan decoder (restart intervals, grey with padding, ...)"
    assert img.flags & 1, "the fixture is not a cut file"
    p, n = C.c_void_p(), C.c_size_t(0)
    L.lep_jpeg_scan_bytes(h, C.byref(p), C.byref(n))
    scan = C.create_string_buffer(C.string_at(p, n.value) + b"\0" * 64, n.value + 64)
    img.scan = C.addressof(scan)
    d = host.desc
    planes = []
    for c in range(d.ncomp):
        b = C.create_string_buffer(d.nblocks(c) * 128)
        planes.append(b)
        img.blocks[c] = C.cast(b, C.c_void_p).value
    rows = (abi.HuffDecRow * (img.mcuv + 1))()
    if stale:
        rows[img.mcuv].bitpos, rows[img.mcuv].aux = stale
    assert emu.emu_huffman_decode_image_simt(C.byref(img), rows, bits, None, None) == 0
    if (rows[img.mcuv].aux >> 8) & 0x3fffff:
        L.lep_jpeg_close(h)
        return "the kernel left the file to the host parser (status %d)" % ((rows[img.mcuv].aux >> 8) & 0x3fffff)
    assert L.lep_jpeg_finish_gpu(h, rows) == 0
    gd = abi.ImageDesc()
    assert L.lep_jpeg_describe(h, C.byref(gd)) == 0
    for c in range(d.ncomp):
        assert gd.coded_blocks[c] == d.coded_blocks[c] and gd.coded_height[c] == d.coded_height[c], (c, gd.coded_blocks[c], d.coded_blocks[c])
        nb = d.coded_blocks[c] * 128
        assert planes[c].raw[:nb] == C.string_at(d.blocks[c], nb), "component %d" % c
    segs = host.plan()
    streams, _ = ob.oracle_encode(d, segs)
    want = host.write_lep(streams)
    arr = (abi.Bytes * len(streams))()
    keep = []
    for i, s in enumerate(streams):
        b = C.create_string_buffer(bytes(s), max(1, len(s)))
        keep.append(b)
        arr[i].data = C.cast(b, C.c_void_p).value
        arr[i].len = arr[i].cap = len(s)
    out = abi.Bytes()
    assert L.lep_jpeg_write_lep(h, 0, arr, len(streams), C.byref(out)) == 0
    got = out.tobytes()
    L.lep_free(out.data)
    L.lep_jpeg_close(h)
    assert got == want
    return True


def test_lane_per_subsequence_decoder_never_leaves_a_stale_final_record(emu):
    """a file cut inside the image's LAST block, subsequences so short that the lane in front of the last one decodes
    that block out of the data's last bits: the last lane stands behind the end and has nothing to write.  The image's final record
    -- an array the launches reuse -- must not be left as an older image had it (here: a made-up `truncated after 7 blocks` with
    status 0): either the kernels' answer is the host parser's or they say the file is not theirs."""
    whole = golden("c420_160x120")[0]
    taken = left = 0
    # (cut, subsequence bits) at which the kernels of round 5 left the planted record standing with status 0 -- found by a sweep over
    # the last 60 bytes x subsequences of 32 .. 2048 bits -- and their neighbourhood
    for cut in (-8, -7, -6, -12, -4):
        for bits in (1056, 1248, 1024, 1280):
            res = _cut_file_through_the_lane_per_subsequence_decoder(emu, whole[:len(whole) + cut], bits, stale=(7, 0x40000000 | 255))
            taken += res is True
            left += isinstance(res, str)
    assert taken + left == 20 and left >= 6


@pytest.mark.parametrize("name", [n for n, _ in _cut_jpegs()])
def test_lane_per_unit_huffman_encoder_restores_files_cut_inside_their_scan(emu, name):
    """The decompress direction of a truncated file on the GPU scan encoder: lep_huff_simt.h stops in front of the first block behind the
    cut and says so (HuffEnd.pad); lep_file_recode_finish takes its bytes when the last thread's byte bound was reached by then -- the file
    comes back byte for byte -- and answers LEP_GPU_PATH_DECLINED otherwise (a shorter scan than the bound: damaged files), which sends the
    caller to the host re-coder.  The .lep is the oracle's for the cut file (== the reference's for the fixtures)."""
    from lepton_amd import abi
    from lepton_amd.codec import LepFile

    jpg = dict(_cut_jpegs())[name]
    L = abi.lib()
    try:
        src = JpegImage(jpg)
    except Exception:
        pytest.skip("the host parser refuses this cut")
    segs0 = src.plan()
    streams, _ = ob.oracle_encode(src.desc, segs0)
    lep = src.write_lep(streams)
    f = LepFile(lep)
    ob.oracle_decode(f.desc, f.segments, f.streams)
    assert f.recode() == jpg                      # the host re-coder (threads) restores it: the baseline of this test
    img = abi.HuffImage()
    segs = (abi.HuffSegment * abi.MAX_SEGMENTS)()
    nseg, ok = C.c_int(0), C.c_int(0)
    assert L.lep_file_recode_plan(f.handle, C.byref(img), segs, C.byref(nseg), C.byref(ok)) == 0
    if not ok.value:   # not for the GPU Huffman encoder (grey, restart intervals, ...): the host re-coder above is the product's path
        assert nseg.value == 0
        return
    assert any(img.trunc_bc[c] for c in range(3)), "the plan does not know the file is cut"
    n = nseg.value
    bufs, arr, ends = [], (abi.Bytes * n)(), (abi.HuffEnd * n)()
    for i in range(n):
        cap = min(segs[i].out_cap, len(jpg) + 1024)
        segs[i].out_cap = cap
        buf = C.create_string_buffer(cap + 8)
        ln = C.c_uint32(0)
        rc = emu.emu_huffman_encode_segment_simt(C.byref(img), C.byref(segs[i]), buf, C.byref(ln), C.byref(ends[i]))
        assert rc == 0, "the lane-per-unit kernel must take every segment of a cut file the plan lets through"
        bufs.append(buf)
        arr[i].data = C.cast(buf, C.c_void_p).value
        arr[i].len = arr[i].cap = ln.value
    out = abi.Bytes()
    rc = L.lep_file_recode_finish(f.handle, arr, ends, n, C.byref(out))
    if rc == 101:
        assert ends[n - 1].pad & 1 and ends[n - 1].attempted < segs[n - 1].out_cap
        return   # the cut was met before the byte bound (LEP_GPU_PATH_DECLINED): the host re-coder's bytes, checked above
    assert rc == 0
    got = out.tobytes()
    L.lep_free(out.data)
    assert got == jpg


REFUSED_RST = (42,)   # EX_UNSUPPORTED_JPEG: how the reference refuses a scan whose restart markers are not where its interval says


def _restored_md5(name):
    """md5 of what the reference restores from its .lep of a damaged fixture of tests/golden/ref (None: the file itself)"""
    from conftest import ref_manifest

    v = ref_manifest()["jpegs"].get(name)
    return v["restored_md5"] if v and not v.get("restored_equals_input", True) else None


def _restart_interval_jpegs():
    """[(name, bytes)]: fixtures with restart intervals (interleaved colour scans: the ones the lane-per-interval form takes), the
    reference's own narrowrst.jpg, PIL files with intervals of one MCU / a few MCUs / one MCU row / several rows, and damaged ones"""
    import io
    import numpy as np
    from PIL import Image
    from conftest import ref_golden
    out = [(n, golden(n)[0]) for n in ("rst_c420_176x112", "lay_mixed_rst_104x72", "lay_ids_pad0_64x64", "lay_440_640x480_2seg")]
    out.append(("narrowrst", ref_golden("narrowrst")[0]))
    rng = np.random.default_rng(77)
    base = np.asarray(Image.fromarray(rng.integers(0, 256, (40, 60, 3), dtype=np.uint8), "RGB").resize((480, 320), Image.BICUBIC)).astype(np.int16)
    img = Image.fromarray(np.clip(base + rng.normal(0, 10, base.shape), 0, 255).astype(np.uint8), "RGB")
    for tag, kw in (("rst_1mcu", dict(restart_marker_blocks=1)), ("rst_7mcu", dict(restart_marker_blocks=7)), ("rst_row", dict(restart_marker_rows=1)),
                    ("rst_3rows_444", dict(restart_marker_rows=3, subsampling="4:4:4")), ("rst_422_optimized", dict(restart_marker_blocks=11, subsampling="4:2:2", optimize=True))):
        buf = io.BytesIO()
        img.save(buf, format="JPEG", quality=88, **{"subsampling": "4:2:0", **kw})
        out.append((tag, buf.getvalue()))
    whole = dict(out)["rst_7mcu"]
    sos = whole.find(b"\xff\xda")
    marks = [i for i in range(sos, len(whole) - 1) if whole[i] == 0xFF and 0xD0 <= whole[i + 1] <= 0xD7]
    dropped = whole[: marks[3]] + whole[marks[3] + 2:]                      # a marker missing: fewer markers than the scan's length asks for
    moved = bytearray(whole); i = marks[5]; moved[i - 3: i + 2] = bytes([moved[i], moved[i + 1]]) + bytes(moved[i - 3: i]); moved = bytes(moved)   # a marker three bytes early
    out += [("rst_marker_dropped", dropped), ("rst_marker_moved", moved)]
    return out


@pytest.mark.parametrize("name", [n for n, _ in _restart_interval_jpegs()])
def test_lane_per_unit_huffman_encoder_on_restart_intervals(emu, name):
    """Scans with restart intervals on lep_huff_simt.h: a unit ends where its interval does and carries the pad bits and the marker, the
    prefix sum counts them, the stuffing pass leaves the markers' FFs alone (recoder.cc:364-400).  For every segment -- under its own
    byte bound and under one that cuts it short, started on an MCU row inside an interval as the hand-offs have it -- the bytes, the
    byte count and the end state are the wavefront-per-segment kernel's, and the file glued from them is the JPEG (a damaged file the
    reference codes with -skipverify restores to what the reference restores: the host re-coder's bytes)"""
    import oracle_binding as ob
    from lepton_amd import abi
    from lepton_amd.codec import LepFile, LeptonError

    jpg = dict(_restart_interval_jpegs())[name]
    try:
        src = JpegImage(jpg)
    except LeptonError as e:   # the reference refuses this file: so does the host parser, with the reference's exit code
        assert e.code in REFUSED_RST, (name, e.code)
        return
    for nthreads in (1, 8):
        plan = src.plan(nthreads)
        streams, _ = ob.oracle_encode(src.desc, plan)
        f = LepFile(src.write_lep(streams, nthreads))
        for c in range(f.desc.ncomp):
            C.memmove(f.desc.blocks[c], src.desc.blocks[c], f.desc.nblocks(c) * 128)
        L = abi.lib()
        img = abi.HuffImage()
        segs = (abi.HuffSegment * abi.MAX_SEGMENTS)()
        nseg, ok = C.c_int(0), C.c_int(0)
        assert L.lep_file_recode_plan(f.handle, C.byref(img), segs, C.byref(nseg), C.byref(ok)) == 0
        if not ok.value:   # not for the GPU scan encoder (narrowrst.jpg: markers the file withheld): the host re-coder's bytes
            assert nseg.value == 0
            _host_path(jpg, _golden_lep(name), _restored_md5(name))
            continue
        assert img.rsti > 0
        for i in range(nseg.value):
            own = min(segs[i].out_cap, len(jpg) + 1024)
            for cap in (own, 100, 37):
                segs[i].out_cap = cap
                outs = []
                for fn in (emu.emu_huffman_encode_segment, emu.emu_huffman_encode_segment_simt):
                    buf = C.create_string_buffer(cap + 8)
                    n = C.c_uint32(0)
                    end = abi.HuffEnd()
                    assert fn(C.byref(img), C.byref(segs[i]), buf, C.byref(n), C.byref(end)) == 0
                    # (`attempted` under a bound that cuts the segment short: the lane-per-unit form counts what its bit buffer kept, enough to say "more than the bound")
                    outs.append((n.value, buf.raw[: n.value], end.attempted if cap == own else end.attempted > cap, end.overhang_byte, end.num_overhang_bits, list(end.last_dc), end.pad))
                assert outs[0] == outs[1], (nthreads, i, cap, outs[0][0], outs[1][0], outs[0][2:], outs[1][2:])
            segs[i].out_cap = own
        got = _emulated_gpu_scan_encode(emu, f)
        assert got is not None and got == f.recode()
        if "marker" not in name:
            assert got == jpg
        # a file that withheld markers (rst_cnt: only the first `rst_limit` markers of the scan are written, the pad bits and the predictor
        # reset stay): both kernels honour the limit the same way
        for limit in (0, 3):
            keep_limit = img.rst_limit
            img.rst_limit = limit
            for i in range(nseg.value):
                outs = []
                for fn in (emu.emu_huffman_encode_segment, emu.emu_huffman_encode_segment_simt):
                    buf = C.create_string_buffer(segs[i].out_cap + 8)
                    n = C.c_uint32(0)
                    end = abi.HuffEnd()
                    assert fn(C.byref(img), C.byref(segs[i]), buf, C.byref(n), C.byref(end)) == 0
                    outs.append((n.value, buf.raw[: n.value], end.attempted, end.overhang_byte, end.num_overhang_bits, list(end.last_dc)))
                assert outs[0] == outs[1], (limit, i, outs[0][0], outs[1][0])
            img.rst_limit = keep_limit
        if nthreads == 1:
            # the same segment cut at MCU rows of our choosing: the second piece starts from the end state of the first (what a hand-off
            # records), inside a restart interval wherever the intervals are not whole rows
            whole = segs[0]
            rows = whole.mcu_row1 - whole.mcu_row0
            for cut_row in sorted({1, rows // 3, rows // 2, rows - 1} - {0, rows}):
                state = None
                pieces = []
                for r0, r1 in ((whole.mcu_row0, whole.mcu_row0 + cut_row), (whole.mcu_row0 + cut_row, whole.mcu_row1)):
                    seg = abi.HuffSegment()
                    C.memmove(C.byref(seg), C.byref(whole), C.sizeof(seg))
                    seg.mcu_row0, seg.mcu_row1, seg.out_cap = r0, r1, len(jpg) + 1024
                    if state is not None:
                        seg.overhang = state.overhang_byte | state.num_overhang_bits << 8
                        for c in range(4):
                            seg.last_dc[c] = state.last_dc[c]
                    outs = []
                    for fn in (emu.emu_huffman_encode_segment, emu.emu_huffman_encode_segment_simt):
                        buf = C.create_string_buffer(seg.out_cap + 8)
                        n = C.c_uint32(0)
                        end = abi.HuffEnd()
                        assert fn(C.byref(img), C.byref(seg), buf, C.byref(n), C.byref(end)) == 0
                        outs.append((n.value, buf.raw[: n.value], end.attempted, end.overhang_byte, end.num_overhang_bits, list(end.last_dc), end.pad))
                    assert outs[0] == outs[1], (cut_row, r0, r1, outs[0][0], outs[1][0], outs[0][2:], outs[1][2:])
                    state = end
                    pieces.append(outs[1][1])
                buf = C.create_string_buffer(len(jpg) + 1032)
                n = C.c_uint32(0)
                end = abi.HuffEnd()
                whole.out_cap = len(jpg) + 1024
                assert emu.emu_huffman_encode_segment(C.byref(img), C.byref(whole), buf, C.byref(n), C.byref(end)) == 0
                assert b"".join(pieces) == buf.raw[: n.value], cut_row


@pytest.mark.parametrize("sub,size", [("4:2:0", (200, 136)), ("4:2:2", (328, 88)), ("4:4:4", (136, 120)), ("4:2:0", (1040, 48))])
def test_lane_per_unit_huffman_encoder_restart_interval_sweep(emu, sub, size):
    """restart intervals of 1 .. 1000 MCUs (shorter than a unit, a unit, a unit and a bit, several units, a row and a bit, longer than the
    scan) x segment cuts at every third MCU row: the lane-per-unit kernels against the wavefront kernel, piece by piece with the end state
    of one piece handed to the next, and the pieces together against the whole"""
    import io
    import numpy as np
    from PIL import Image
    import oracle_binding as ob
    from lepton_amd import abi
    from lepton_amd.codec import LepFile

    rng = np.random.default_rng(size[0] * 7 + size[1])
    base = np.asarray(Image.fromarray(rng.integers(0, 256, (size[1] // 8, size[0] // 8, 3), dtype=np.uint8), "RGB").resize(size, Image.BICUBIC)).astype(np.int16)
    pic = Image.fromarray(np.clip(base + rng.normal(0, 14, base.shape), 0, 255).astype(np.uint8), "RGB")
    L = abi.lib()
    for rsti in (1, 2, 3, 7, 8, 9, 16, 17, 63, 64, 65, 1000):
        buf = io.BytesIO()
        pic.save(buf, format="JPEG", quality=int(rng.integers(60, 97)), subsampling=sub, restart_marker_blocks=rsti)
        jpg = buf.getvalue()
        src = JpegImage(jpg)
        streams, _ = ob.oracle_encode(src.desc, src.plan(1))
        f = LepFile(src.write_lep(streams, 1))
        for c in range(f.desc.ncomp):
            C.memmove(f.desc.blocks[c], src.desc.blocks[c], f.desc.nblocks(c) * 128)
        img = abi.HuffImage()
        segs = (abi.HuffSegment * abi.MAX_SEGMENTS)()
        nseg, ok = C.c_int(0), C.c_int(0)
        assert L.lep_file_recode_plan(f.handle, C.byref(img), segs, C.byref(nseg), C.byref(ok)) == 0 and ok.value and nseg.value == 1
        assert img.rsti == rsti
        whole = segs[0]
        whole.out_cap = len(jpg) + 1024
        wbuf = C.create_string_buffer(whole.out_cap + 8)
        wn = C.c_uint32(0)
        wend = abi.HuffEnd()
        assert emu.emu_huffman_encode_segment(C.byref(img), C.byref(whole), wbuf, C.byref(wn), C.byref(wend)) == 0
        cuts = list(range(whole.mcu_row0, whole.mcu_row1, 3)) + [whole.mcu_row1]
        state, pieces = None, []
        for r0, r1 in zip(cuts, cuts[1:]):
            seg = abi.HuffSegment()
            C.memmove(C.byref(seg), C.byref(whole), C.sizeof(seg))
            seg.mcu_row0, seg.mcu_row1 = r0, r1
            if state is not None:
                seg.overhang = state.overhang_byte | state.num_overhang_bits << 8
                for c in range(4):
                    seg.last_dc[c] = state.last_dc[c]
            outs = []
            for fn in (emu.emu_huffman_encode_segment, emu.emu_huffman_encode_segment_simt):
                b = C.create_string_buffer(seg.out_cap + 8)
                n = C.c_uint32(0)
                end = abi.HuffEnd()
                assert fn(C.byref(img), C.byref(seg), b, C.byref(n), C.byref(end)) == 0
                outs.append((n.value, b.raw[: n.value], end.attempted, end.overhang_byte, end.num_overhang_bits, list(end.last_dc), end.pad))
            assert outs[0] == outs[1], (rsti, r0, r1, outs[0][0], outs[1][0], outs[0][2:], outs[1][2:])
            state = end
            pieces.append(outs[1][1])
        assert b"".join(pieces) == wbuf.raw[: wn.value], rsti
        assert _emulated_gpu_scan_encode(emu, f) == jpg, rsti


@pytest.mark.parametrize("name", [n for n, _ in _restart_interval_jpegs()])
def test_lane_per_restart_interval_huffman_decoder(emu, name):
    """Scans with restart intervals on lep_huffdec_simt.h: the markers' positions travel behind the scan bytes (LEP_HUFFDEC_RST_TABLE) and
    every interval is decoded by a lane of its own -- frame, hand-off records and pad bits must be the host parser's (the .lep written from
    them == the host parser's == the reference's for the fixtures), or the kernel reports a status and the file goes the single-wave
    kernel's / host parser's way; a file whose markers are not where its restart interval says is not flagged at all"""
    from lepton_amd import abi
    from lepton_amd.codec import LeptonError

    jpg = dict(_restart_interval_jpegs())[name]
    L = abi.lib()
    try:
        host = JpegImage(jpg)
    except LeptonError:
        host = None                                  # the reference refuses the damaged file: so must every path of ours
    h = C.c_void_p()
    img = abi.HuffDecImage()
    ok = C.c_int(0)
    rc = L.lep_jpeg_open_gpu(jpg, len(jpg), C.byref(h), C.byref(img), C.byref(ok))
    if rc:
        assert host is None
        return
    if not ok.value:   # not for the GPU scan decoder: the host parser's path is the product's
        L.lep_jpeg_close(h)
        assert host is not None
        _host_path(jpg, _golden_lep(name), _restored_md5(name))
        return
    assert img.rsti > 0
    damaged = name in ("rst_marker_dropped", "rst_marker_moved")
    if name == "rst_marker_dropped":
        assert not (img.flags & 2), "a scan with a marker missing must not be flagged LEP_HUFFDEC_RST_TABLE"
    if not (img.flags & 2):
        L.lep_jpeg_close(h)
        pytest.skip("markers not where the restart interval says: the single-wave kernel's")
    p, n = C.c_void_p(), C.c_size_t(0)
    L.lep_jpeg_scan_bytes(h, C.byref(p), C.byref(n))
    rp, rn = C.POINTER(C.c_uint32)(), C.c_size_t(0)
    L.lep_jpeg_scan_restarts(h, C.byref(rp), C.byref(rn))
    assert rn.value == (img.mcuc - 1) // img.rsti
    room = (n.value + 64 + 15) & ~15
    table = bytes(C.cast(rp, C.POINTER(C.c_uint8 * (4 * rn.value))).contents) if rn.value else b""
    scan = C.create_string_buffer(C.string_at(p, n.value) + b"\0" * (room - n.value) + table + b"\0" * 64, room + len(table) + 64)
    assert C.addressof(scan) % 8 == 0
    img.scan = C.addressof(scan)
    d = host.desc if host else None
    gd = abi.ImageDesc()
    planes = []
    ncomp = img.ncomp
    for c in range(ncomp):
        b = C.create_string_buffer(img.bch[c] * img.vs[c] * img.mcuv * 128)
        planes.append(b)
        img.blocks[c] = C.cast(b, C.c_void_p).value
    rows = (abi.HuffDecRow * (img.mcuv + 1))()
    assert emu.emu_huffman_decode_image_simt(C.byref(img), rows, 8192, None, None) == 0
    status = (rows[img.mcuv].aux >> 8) & 0x3fffff
    if damaged or host is None:
        assert status != 0 or L.lep_jpeg_finish_gpu(h, rows) != 0 or host is not None, "a damaged scan slipped through"
    if status:
        L.lep_jpeg_close(h)
        assert damaged or host is None, "kernel reported an irregular scan on a clean fixture (status %d)" % status
        return
    if L.lep_jpeg_finish_gpu(h, rows) != 0:
        L.lep_jpeg_close(h)
        assert damaged or host is None
        return
    assert host is not None
    for c in range(d.ncomp):
        assert planes[c].raw[: d.nblocks(c) * 128] == C.string_at(d.blocks[c], d.nblocks(c) * 128), "component %d" % c
    segs = host.plan()
    streams, _ = ob.oracle_encode(d, segs)
    want = host.write_lep(streams)
    arr = (abi.Bytes * len(streams))()
    keep = []
    for i, s in enumerate(streams):
        b = C.create_string_buffer(bytes(s), max(1, len(s)))
        keep.append(b)
        arr[i].data = C.cast(b, C.c_void_p).value
        arr[i].len = arr[i].cap = len(s)
    out = abi.Bytes()
    assert L.lep_jpeg_write_lep(h, 0, arr, len(streams), C.byref(out)) == 0
    got = out.tobytes()
    L.lep_free(out.data)
    L.lep_jpeg_close(h)
    assert got == want
