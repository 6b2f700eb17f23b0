#!/usr/bin/env python3
"""What a band boundary of the resumable decoder costs (lep_gpu_decode_rows_*, lep_decode_v4_rows_kernel) on 4K images: device-resident
frames and streams, launches of 8 segments (one image) and of 8 x --images segments.

  one-shot   lep_gpu_decode_device + sync, for the library under test and -- with --parent <path of another build of the library> -- for
             that build, loaded beside it in the same process and run in turn (same kernel in both: the difference is the spread)
  session    begin .. advance until nothing runs .. end, at every --bands value (0 = to the end); `first` is the time from begin to the
             first advance's return: what a caller waits for the first rows

--repeats alternating rounds over all variants; the table gives the median and the range of each.  One JSON line at the end."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lepton_amd import abi, corpus  # noqa: E402
from lepton_amd.codec import GpuCodec, JpegImage  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bands", default="0,1,4,16")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent", default="")
    ap.add_argument("--workers", type=int, default=16)
    a = ap.parse_args()
    bands = [int(b) for b in a.bands.split(",")]
    jpgs = corpus.make_corpus(a.images, a.width, a.height, 1234, workers=a.workers)   # (the process pool ends before the GPU is opened)
    L = abi.lib()
    codec = GpuCodec(0)
    h = codec.handle
    imgs = [JpegImage(j) for j in jpgs]
    plans = [im.plan() for im in imgs]
    streams = []
    for i in range(0, len(imgs), 16):
        streams += codec.encode(imgs[i:i + 16], plans[i:i + 16])

    def dmalloc(n):
        p = C.c_void_p()
        assert L.lep_gpu_malloc(h, n, C.byref(p)) == 0
        return p

    dev = (abi.ImageDesc * len(imgs))(*[im.desc for im in imgs])
    for i, im in enumerate(imgs):
        for c in range(im.desc.ncomp):
            dev[i].blocks[c] = dmalloc(im.desc.nblocks(c) * 128 + 256).value

    def launch_of(nimg):
        flat = [abi.Segment(i, s.luma_y_start, s.luma_y_end, s.is_last) for i in range(nimg) for s in plans[i]]
        sts = [st for i in range(nimg) for st in streams[i]]
        blob, offs = b"", [0]
        for st in sts:
            blob += st + bytes(-len(st) % 256)
            offs.append(len(blob))
        n = len(flat)
        d_streams, d_lens, d_status = dmalloc(len(blob) + 256), dmalloc(4 * n), dmalloc(4 * n)
        assert L.lep_gpu_memcpy_h2d(h, d_streams, blob, len(blob)) == 0
        assert L.lep_gpu_memcpy_h2d(h, d_lens, (C.c_uint32 * n)(*[len(st) for st in sts]), 4 * n) == 0
        return dict(nimg=nimg, nseg=n, segs=(abi.Segment * n)(*flat), offs=(C.c_uint64 * (n + 1))(*offs), d_streams=d_streams, d_lens=d_lens,
                    d_status=d_status, status=(C.c_int32 * n)(), prog=(abi.DecodeProgress * n)())

    def one_shot(lib, handle, w):
        t0 = time.perf_counter()
        assert lib.lep_gpu_decode_device(handle, dev, w["nimg"], w["segs"], w["nseg"], w["d_streams"], w["offs"], w["d_lens"], w["d_status"], None) == 0
        assert lib.lep_gpu_sync(handle) == 0
        t = time.perf_counter() - t0
        assert L.lep_gpu_memcpy_d2h(h, w["status"], w["d_status"], 4 * w["nseg"]) == 0 and not any(w["status"])
        return {"total_ms": t * 1e3}

    def session(w, band):
        running, advances = C.c_int(1), 0
        t0 = time.perf_counter()
        assert L.lep_gpu_decode_rows_begin(h, dev, w["nimg"], w["segs"], w["nseg"], w["d_streams"], w["offs"], w["d_lens"], None) == 0
        first = None
        while running.value > 0:
            assert L.lep_gpu_decode_rows_advance(h, band, w["prog"], C.byref(running)) == 0
            advances += 1
            if first is None:
                first = time.perf_counter() - t0
        assert L.lep_gpu_decode_rows_end(h) == 0
        t = time.perf_counter() - t0
        assert all(w["prog"][k].status == 0 for k in range(w["nseg"]))
        return {"total_ms": t * 1e3, "first_ms": first * 1e3, "advances": advances}

    variants = [("one-shot, this build", lambda w: one_shot(L, h, w))]
    if a.parent:
        P = C.CDLL(a.parent)
        vp = C.c_void_p
        P.lep_gpu_create.argtypes = [C.c_int, C.POINTER(vp)]
        P.lep_gpu_decode_device.argtypes = L.lep_gpu_decode_device.argtypes
        P.lep_gpu_sync.argtypes = [vp]
        ph = vp()
        assert P.lep_gpu_create(0, C.byref(ph)) == 0
        variants.insert(0, ("one-shot, parent build", lambda w: one_shot(P, ph, w)))
    for b in bands:
        variants.append(("session, band %d" % b, lambda w, b=b: session(w, b)))

    out = {}
    for nimg in sorted({1, a.images}):
        w = launch_of(nimg)
        for _, fn in variants:     # warm-up: workspaces grow, code objects load
            fn(w)
        runs = {name: [] for name, _ in variants}
        for _ in range(a.repeats):
            for name, fn in variants:
                runs[name].append(fn(w))
        out["%d segments" % w["nseg"]] = runs
        print("%d segments (%d image%s), %d alternating rounds; ms: median (min .. max)" % (w["nseg"], nimg, "" if nimg == 1 else "s", a.repeats))
        for name, _ in variants:
            r = runs[name]

            def col(key):
                v = [x[key] for x in r]
                return "%8.2f (%8.2f .. %8.2f)" % (statistics.median(v), min(v), max(v))

            line = "  %-24s total %s" % (name, col("total_ms"))
            if "first_ms" in r[0]:
                line += "   first %s   advances %d" % (col("first_ms"), r[0]["advances"])
            print(line)
    print(json.dumps({"images": a.images, "size": [a.width, a.height], "results": out}))


if __name__ == "__main__":
    main()
