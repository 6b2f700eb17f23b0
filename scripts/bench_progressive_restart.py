#!/usr/bin/env python3
"""Progressive files WITH restart intervals through the batch compressor and the progressive scan decoders: 256 x 4K files (32 distinct,
written by Pillow from seeded pictures; nothing is downloaded), two corpora -- a marker per MCU row, and an interval of 516 blocks (the
larger of the two intervals of the reference's phone images).  Per corpus: compress_batch warm, --repeats timed runs
(median and min, MB/s), and the scan-decode time alone -- lep_gpu_huffman_progressive_decode_device on the same files resident on the
device, from lep_gpu_last_kernel_ms.  One JSON line per corpus.

--write adds the other direction: decompress_batch warm with --repeats timed runs, and the scan WRITE alone on resident frames
(lep_gpu_huffman_progressive_encode_device, from lep_gpu_last_kernel_ms; duplicates of a picture share its frame on the device).
--write-only leaves the compress leg out.

The baseline is ANOTHER BUILD of the library (LEP_LIB_PATH=<the parent commit's liblepton_mi355x.so>), alternated with this one in the
same visit; LEP_HUFFPROGDEC_RST=0 on this build is a convenience, not the baseline.  --cache DIR keeps the corpus between processes.

--corpus plain: 256 x 4K progressive files WITHOUT restart intervals from bench.py's own generator (lepton_amd.corpus.make_corpus, the
seed of its `progressive` corpus, 8 distinct) -- what the window decoder's whole-file path is measured on when that kernel changes;
--decode-only leaves the timed compress_batch runs out (one warm call still checks that every file takes the scan kernels)."""
import argparse
import ctypes as C
import io
import json
import os
import statistics
import struct
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CORPORA = {"rows_1": dict(restart_marker_rows=1), "blocks_516": dict(restart_marker_blocks=516),
           "blocks_5": dict(restart_marker_blocks=5),    # (blocks_5: a marker per five blocks, about 26,000 units per luma scan; not part of "both")
           "none": dict(),                               # (none: the same pictures without an interval, for --write-only; not part of "both")
           "plain": None}                                # (plain: bench.py's progressive corpus, no interval; not part of "both")
BOTH = ["blocks_516", "rows_1"]


def picture(args):
    w, h, seed, restart = args
    from PIL import Image

    rng = np.random.default_rng(seed)
    base = Image.fromarray(rng.integers(0, 256, (max(2, h // 64), max(2, w // 64), 3), dtype=np.uint8), "RGB").resize((w, h), Image.BICUBIC)
    tex = Image.fromarray(rng.integers(0, 48, (max(2, h // 4), max(2, w // 4), 3), dtype=np.uint8), "RGB").resize((w, h), Image.BILINEAR)
    a = np.clip(np.asarray(base, dtype=np.int16) + np.asarray(tex, dtype=np.int16) - 24, 0, 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(a, "RGB").save(buf, format="JPEG", quality=90, subsampling=2, progressive=True, **restart)
    return buf.getvalue()


def corpus(name, w, h, distinct, cache):
    if CORPORA[name] is None:                            # bench.py's generator and seed (its `progressive` extra: 30001 + 1000 * 2)
        from lepton_amd import corpus as bench_corpus

        files = [os.path.join(cache, "%s_%dx%d_%02d.jpg" % (name, w, h, i)) for i in range(distinct)] if cache else []
        if files and all(os.path.exists(p) for p in files):
            return [open(p, "rb").read() for p in files]
        made = bench_corpus.make_corpus(distinct, w, h, 32001, progressive=True)
        for p, j in zip(files, made):
            os.makedirs(cache, exist_ok=True)
            open(p, "wb").write(j)
        return made
    out = []
    missing = []
    for i in range(distinct):
        p = os.path.join(cache, "%s_%dx%d_%02d.jpg" % (name, w, h, i)) if cache else None
        if p and os.path.exists(p):
            out.append(open(p, "rb").read())
        else:
            out.append(None); missing.append(i)
    if missing:
        with ProcessPoolExecutor(max_workers=min(16, len(missing))) as ex:
            made = list(ex.map(picture, [(w, h, 5000 + i, CORPORA[name]) for i in missing]))
        for i, j in zip(missing, made):
            out[i] = j
            if cache:
                os.makedirs(cache, exist_ok=True)
                open(os.path.join(cache, "%s_%dx%d_%02d.jpg" % (name, w, h, i)), "wb").write(j)
    return out


def resident(L, g, jpgs):
    """every file's scans on the device as the batch pipeline lays them out; returns (descriptors, n, frames pointer, frame bytes, rows pointer)"""
    from lepton_amd import abi

    has_tables = hasattr(L, "lep_jpeg_scan_restarts_of")
    all_scans, arena, frames, nrec, handles = [], bytearray(), 0, 0, []
    for jpg in jpgs:
        h, plan1, ok = C.c_void_p(), abi.HuffDecImage(), C.c_int(0)
        assert L.lep_jpeg_open_gpu(jpg, len(jpg), C.byref(h), C.byref(plan1), C.byref(ok)) == 0 and not ok.value
        scans = (abi.HuffProgDecScan * 64)()
        nscan, need, ok2 = C.c_int(0), C.c_int(0), C.c_int(0)
        assert L.lep_jpeg_open_gpu_progressive(h, scans, 64, C.byref(nscan), C.byref(need), C.byref(ok2)) == 0 and ok2.value
        p, n = C.c_void_p(), C.c_size_t(0)
        L.lep_jpeg_scan_bytes(h, C.byref(p), C.byref(n))
        raw = C.string_at(p, n.value)
        sizes = [scans[0].t.bch[c] * scans[0].bcv[c] * 128 for c in range(scans[0].t.ncomp)]
        for i in range(nscan.value):
            sc = abi.HuffProgDecScan.from_buffer_copy(scans[i])
            off, ln = sc.t.scan or 0, sc.t.scan_len
            sc.t.scan = len(arena)
            arena += raw[off:off + ln] + bytes(((ln + 80 + 15) & ~15) - ln)
            if sc.t.flags & 2:
                assert has_tables
                rp, rn = C.POINTER(C.c_uint32)(), C.c_size_t(0)
                L.lep_jpeg_scan_restarts_of(h, i, C.byref(rp), C.byref(rn))
                arena += struct.pack("<%dI" % rn.value, *rp[:rn.value])
                arena += bytes(-len(arena) % 16)
            at = frames
            for c in range(sc.t.ncomp):
                sc.t.blocks[c] = at
                at += sizes[c]
            sc.t.rows_off += nrec
            sc.result_off += nrec
            all_scans.append(sc)
        frames += (sum(sizes) + 255) & ~255
        nrec += need.value
        handles.append(h)
    arena += bytes(256)
    d_scan, d_frames, d_rows = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.lep_gpu_malloc(g, len(arena), C.byref(d_scan)) == 0 and L.lep_gpu_malloc(g, frames, C.byref(d_frames)) == 0
    assert L.lep_gpu_malloc(g, (nrec + 4) * C.sizeof(abi.HuffDecRow), C.byref(d_rows)) == 0
    assert L.lep_gpu_memcpy_h2d(g, d_scan, bytes(arena), len(arena)) == 0
    arr = (abi.HuffProgDecScan * len(all_scans))(*all_scans)
    for sc in arr:
        sc.t.scan = d_scan.value + (sc.t.scan or 0)
        for c in range(sc.t.ncomp):
            sc.t.blocks[c] = d_frames.value + (sc.t.blocks[c] or 0)
    for h in handles:
        L.lep_jpeg_close(h)
    return arr, len(all_scans), d_frames, frames, d_rows, nrec, (d_scan, d_frames, d_rows)


def resident_frames(L, g, distinct, files):
    """the distinct pictures' frames on the device and the plan that writes every scan of `files` files again (lep_jpeg_plan_progressive_check)"""
    from lepton_amd import abi
    from lepton_amd.codec import JpegImage

    per, mem = [], []
    for jpg in distinct:
        src = JpegImage(jpg)
        img, scans = abi.HuffProgImage(), (abi.HuffProgScan * 64)()
        first, flen = (C.c_uint32 * 64)(), (C.c_uint32 * 64)()
        n, ok = C.c_int(0), C.c_int(0)
        assert L.lep_jpeg_plan_progressive_check(src.handle, len(jpg), C.byref(img), scans, first, flen, 64, C.byref(n), C.byref(ok)) == 0 and ok.value
        for c in range(src.desc.ncomp):
            nbytes = src.desc.nblocks(c) * 128
            d = C.c_void_p()
            assert L.lep_gpu_malloc(g, nbytes, C.byref(d)) == 0
            assert L.lep_gpu_memcpy_h2d(g, d, C.string_at(src.desc.blocks[c], nbytes), nbytes) == 0
            img.blocks[c] = d.value
            mem.append(d)
        per.append((img, [(abi.HuffProgScan.from_buffer_copy(scans[i]), flen[i], jpg[first[i]: first[i] + flen[i]]) for i in range(n.value)]))
    imgs, all_scans, want = [], [], []
    out_total = corr_total = 0
    for k in range(files):
        img, scans = per[k % len(per)]
        imgs.append(img)
        for sc0, ln, own in scans:
            sc = abi.HuffProgScan.from_buffer_copy(sc0)
            sc.image = k
            sc.out_cap = min(sc.out_cap, ln + 64)
            sc.out_off = out_total
            out_total += (sc.out_cap + 15) & ~15
            sc.corr_off = corr_total
            corr_total += sc.corr_cap
            all_scans.append(sc); want.append(own)
    return (abi.HuffProgImage * files)(*imgs), (abi.HuffProgScan * len(all_scans))(*all_scans), len(all_scans), out_total + 64, corr_total + 8, mem, want


def write_leg(L, codec, distinct, jpgs, repeats):
    """decompress_batch and the scan write alone; every scan's bytes are held against the file's own"""
    g = codec.handle
    leps, st, _ = codec.compress_batch(distinct)
    assert st == [0] * len(distinct)
    leps = [leps[i % len(distinct)] for i in range(len(jpgs))]
    back, st, stats = codec.decompress_batch(leps)                      # warm
    assert st == [0] * len(leps) and back == jpgs, "a file of the corpus was not restored"
    assert stats["gpu_huffman_files"] == len(leps), "a file of the corpus went to the host re-coder"
    secs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        _, st, _ = codec.decompress_batch(leps)
        secs.append(time.perf_counter() - t0)
        assert st == [0] * len(leps)
    imgs, scans, n, out_bytes, corr_words, mem, want = resident_frames(L, g, distinct, len(jpgs))
    d_out, d_corr, d_len = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.lep_gpu_malloc(g, out_bytes, C.byref(d_out)) == 0 and L.lep_gpu_malloc(g, corr_words * 4, C.byref(d_corr)) == 0 and L.lep_gpu_malloc(g, n * 4 + 16, C.byref(d_len)) == 0
    ms, kernel = [], ""
    for rep in range(repeats + 1):                                      # (the first one warm)
        assert L.lep_gpu_huffman_progressive_encode_device(g, imgs, len(jpgs), scans, n, d_out, d_corr, d_len, None) == 0, codec.last_error()
        assert L.lep_gpu_sync(g) == 0, codec.last_error()
        if rep:
            ms.append(L.lep_gpu_last_kernel_ms(g))
        kernel = L.lep_gpu_last_kernel_name(g).decode()
    forms = None
    if hasattr(L, "lep_gpu_huffman_progressive_encode_forms"):
        counts = (C.c_uint32 * 4)()
        L.lep_gpu_huffman_progressive_encode_forms(g, C.byref(counts))
        forms = list(counts)
    out, lens = C.create_string_buffer(out_bytes), (C.c_uint32 * n)()
    assert L.lep_gpu_memcpy_d2h(g, out, d_out, out_bytes) == 0 and L.lep_gpu_memcpy_d2h(g, lens, d_len, n * 4) == 0
    got = memoryview(out)                                               # (out.raw would copy the whole arena once per scan)
    wrong = sum(1 for i in range(n) if lens[i] >= 0x80000000 or bytes(got[scans[i].out_off: scans[i].out_off + lens[i]]) != want[i])
    for m in mem + [d_out, d_corr, d_len]:
        L.lep_gpu_free(g, m)
    nbytes = sum(map(len, jpgs))
    return {"decompress_batch_s": {"median": round(statistics.median(secs), 4), "min": round(min(secs), 4)},
            "decompress_MB_s": {"median": round(nbytes / statistics.median(secs) / 1e6, 1), "best": round(nbytes / min(secs) / 1e6, 1)},
            "scan_write_ms": {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}, "scan_write_kernel": kernel,
            "scans_written": n, "scans_by_form": forms, "scans_not_the_files_own": wrong, "knob_LEP_HUFFPROG_SIMT_RST": os.environ.get("LEP_HUFFPROG_SIMT_RST")}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--distinct", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--corpus", choices=sorted(CORPORA) + ["both"], default="both")
    ap.add_argument("--cache", default=None)
    ap.add_argument("--write", action="store_true", help="add the write leg: decompress_batch and the scan write alone")
    ap.add_argument("--write-only", action="store_true", help="the write leg without the compress leg")
    ap.add_argument("--decode-only", action="store_true", help="the scan decode alone: no timed compress_batch runs")
    ap.add_argument("--label", default=os.environ.get("LEP_LIB_PATH") and "LEP_LIB_PATH" or "this build")
    a = ap.parse_args()
    assert a.repeats >= 5, "at least 5 repeats"
    from lepton_amd import abi
    from lepton_amd.codec import GpuCodec

    L = abi.lib()
    codec = GpuCodec(0)
    for name in (BOTH if a.corpus == "both" else [a.corpus]):
        distinct = corpus(name, a.width, a.height, a.distinct, a.cache)
        jpgs = [distinct[i % len(distinct)] for i in range(a.files)]
        nbytes = sum(map(len, jpgs))
        if a.write_only:
            print(json.dumps(dict({"corpus": name, "label": a.label, "library": abi.LIB_PATH, "files": a.files, "distinct": a.distinct, "size": [a.width, a.height], "jpeg_bytes": nbytes,
                                   "repeats": a.repeats}, **write_leg(L, codec, distinct, jpgs, a.repeats))), flush=True)
            continue
        _, st, stats = codec.compress_batch(jpgs)                       # warm: staging, workspaces
        assert st == [0] * len(jpgs), "a file of the corpus was refused"
        assert stats["gpu_huffman_files"] == len(jpgs), "a file of the corpus went to the host parser"
        secs = []
        for _ in range(0 if a.decode_only else a.repeats):
            t0 = time.perf_counter()
            _, st, _ = codec.compress_batch(jpgs)
            secs.append(time.perf_counter() - t0)
            assert st == [0] * len(jpgs)
        g = codec.handle
        arr, n, d_frames, fbytes, d_rows, nrec, mem = resident(L, g, jpgs)
        ms, kernel = [], ""
        for rep in range(a.repeats + 1):                                # (the first one warm)
            assert L.lep_gpu_memset(g, d_frames, 0, fbytes) == 0
            assert L.lep_gpu_huffman_progressive_decode_device(g, arr, n, d_rows, None) == 0, codec.last_error()
            assert L.lep_gpu_sync(g) == 0, codec.last_error()
            if rep:
                ms.append(L.lep_gpu_last_kernel_ms(g))
            kernel = L.lep_gpu_last_kernel_name(g).decode()
        rows = (abi.HuffDecRow * (nrec + 4))()
        assert L.lep_gpu_memcpy_d2h(g, rows, d_rows, (nrec + 4) * C.sizeof(abi.HuffDecRow)) == 0
        refused = sum(1 for sc in arr if rows[sc.result_off].aux >> 8)
        for m in mem:
            L.lep_gpu_free(g, m)
        written = write_leg(L, codec, distinct, jpgs, a.repeats) if a.write else {}
        print(json.dumps({"corpus": name, "label": a.label, "library": abi.LIB_PATH, "files": a.files, "distinct": a.distinct, "size": [a.width, a.height], "jpeg_bytes": nbytes,
                          "knob_LEP_HUFFPROGDEC_RST": os.environ.get("LEP_HUFFPROGDEC_RST"), "repeats": a.repeats, **written,
                          **({} if a.decode_only else {
                              "compress_batch_s": {"median": round(statistics.median(secs), 4), "min": round(min(secs), 4)},
                              "compress_MB_s": {"median": round(nbytes / statistics.median(secs) / 1e6, 1), "best": round(nbytes / min(secs) / 1e6, 1)}}),
                          "scan_decode_ms": {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}, "scan_decode_kernel": kernel,
                          "scans": n, "scans_with_a_status": refused}), flush=True)
    codec.close()


if __name__ == "__main__":
    main()
