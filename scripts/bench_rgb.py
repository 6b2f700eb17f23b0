#!/usr/bin/env python3
"""Pixels from .lep files (lep_rgb.h): lep_gpu_rgb_device's kernel on resident planes, and lep_decompress_rgb against
lep_decompress_planes at scale 1 and lep_decompress on one file.  DESIGN 4.6's method: kernel times are HIP events around the launch
(lep_gpu_last_kernel_ms), `--images` copies of one 4K 4:2:0 plane set resident in HBM, one launch for all of them, 3 warm-up launches,
then 20 timed ones; whole-file times are a host clock around calls that end synchronised, the three calls alternating, 2 warm-ups, then
7 each.  Prints the lines that profiles/ keeps; --out writes them to a file as well.

    python scripts/bench_rgb.py [--images 64] [--out profiles/NAME.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_TBS = 8.0          # DESIGN 4.5's HBM rate


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import __graft_entry__ as g

    g.build()
    import rgb_ref
    from lepton_amd import abi, corpus
    from lepton_amd.codec import GpuCodec, _check

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    codec = GpuCodec(0)
    L, h = codec._L, codec.handle
    jpg = corpus.synth_jpeg(a.width, a.height, seed=7)
    lep = codec.compress(jpg)
    res = codec.decompress_planes(lep, 1)
    w, ht, n = res["width"], res["height"], res["ncomp"]
    say("file: corpus.synth_jpeg(%d, %d, seed=7), 4:2:0 baseline, %d JPEG bytes, %d .lep bytes; planes %s, pitches %s"
        % (a.width, a.height, len(jpg), len(lep), list(zip(res["plane_width"], res["plane_height"])), res["pitch"]))
    planes = [np.frombuffer(p, dtype=np.uint8).reshape(res["plane_height"][c], res["pitch"][c]) for c, p in enumerate(res["planes"])]
    want = rgb_ref.pixels(planes, w, ht, res["h_samp"], res["v_samp"], True)

    # -- the kernel: `images` plane sets and outputs resident, one launch
    geo = rgb_ref.geometry(w, ht, res["h_samp"], res["v_samp"])
    set_bytes = sum(len(p) for p in res["planes"])
    used_bytes = sum(dw * dh for dw, dh, _, _ in geo)
    out_bytes = w * ht * 3
    owned = []

    def dmalloc(k):
        p = C.c_void_p()
        _check(L.lep_gpu_malloc(h, k, C.byref(p)), "lep_gpu_malloc")
        owned.append(p)
        return p

    try:
        d_planes, d_out = dmalloc(set_bytes * a.images), dmalloc(out_bytes * a.images)
        blob = b"".join(res["planes"])
        offs = np.cumsum([0] + [len(p) for p in res["planes"]])
        recs = (abi.RgbImage * a.images)()
        for i in range(a.images):
            _check(L.lep_gpu_memcpy_h2d(h, d_planes.value + i * set_bytes, blob, set_bytes), "h2d")
            r = recs[i]
            r.width, r.height, r.ncomp, r.convert = w, ht, n, 1
            for c in range(n):
                r.h_samp[c], r.v_samp[c], r.plane_pitch[c] = res["h_samp"][c], res["v_samp"][c], res["pitch"][c]
                r.d_plane[c] = d_planes.value + i * set_bytes + int(offs[c])
            r.d_rgb, r.rgb_pitch, r.y_first, r.y_end = d_out.value + i * out_bytes, w * 3, 0, ht
        _check(L.lep_gpu_memset(h, d_out, 0xEE, out_bytes * a.images), "memset")
        ms = []
        for k in range(a.warmup + a.launches):
            _check(L.lep_gpu_rgb_device(h, recs, a.images, None), "lep_gpu_rgb_device [%s]" % codec.last_error())
            t = L.lep_gpu_last_kernel_ms(h)
            if k >= a.warmup:
                ms.append(t)
        _check(L.lep_gpu_sync(h), "sync")
        equal = []
        for i in (0, a.images - 1):
            host = C.create_string_buffer(out_bytes)
            _check(L.lep_gpu_memcpy_d2h(h, host, d_out.value + i * out_bytes, out_bytes), "d2h")
            equal.append(bool(np.array_equal(np.frombuffer(host.raw, dtype=np.uint8).reshape(ht, w, 3), want)))
        med = statistics.median(ms)
        moved = (used_bytes + out_bytes) * a.images
        # rows of a vertically subsampled component feed two output rows: what the lanes request from L2
        requested = sum(dw * dh * fv for dw, dh, _, fv in geo) * a.images
        say("%s, %d images: %.1f MB of planes read (each sample once), %.1f MB written; kernel ms over %d launches after %d warm-ups: min %.3f median %.3f max %.3f; "
            "the bytes at %g TB/s (DESIGN 4.5's HBM rate): %.3f ms; achieved %.2f TB/s = %.2f at the median; %.1f MB requested by the lanes (rows of a vertically "
            "subsampled component twice); pixels of images 0 and %d equal tests/rgb_ref.py: %s"
            % (L.lep_gpu_last_kernel_name(h).decode(), a.images, used_bytes * a.images / 1e6, out_bytes * a.images / 1e6, a.launches, a.warmup, min(ms), med, max(ms),
               HBM_TBS, moved / (HBM_TBS * 1e12) * 1e3, moved / (med * 1e-3) / 1e12, moved / (med * 1e-3) / 1e12 / HBM_TBS, requested / 1e6, a.images - 1, equal))
        if not all(equal):
            raise SystemExit("the kernel's pixels differ from tests/rgb_ref.py")
    finally:
        for p in owned:
            L.lep_gpu_free(h, p)

    # -- whole files
    calls = {"lep_decompress": lambda: codec.decompress(lep), "lep_decompress_planes scale 1": lambda: codec.decompress_planes(lep, 1),
             "lep_decompress_rgb": lambda: codec.decompress_rgb(lep)}
    got = codec.decompress_rgb(lep)
    if not np.array_equal(np.frombuffer(got["pixels"], dtype=np.uint8).reshape(ht, w, 3), want):
        raise SystemExit("lep_decompress_rgb's pixels differ from tests/rgb_ref.py")
    times = {k: [] for k in calls}
    for k in range(2 + a.calls):
        for name, call in calls.items():
            t0 = time.perf_counter()
            call()
            if k >= 2:
                times[name].append((time.perf_counter() - t0) * 1e3)
    for name, t in times.items():
        say("%s, one file, wall ms over %d calls after 2 warm-ups, the three calls alternating: min %.1f median %.1f max %.1f" % (name, a.calls, min(t), statistics.median(t), max(t)))
    say("bytes down: lep_decompress copies the %.1f MB frame to the host and writes %.2f MB of JPEG there; planes at scale 1: %.1f MB; pixels: %.1f MB"
        % (sum(pw * ph for pw, ph in zip(res["plane_width"], res["plane_height"])) * 2 / 1e6, len(jpg) / 1e6, set_bytes / 1e6, out_bytes / 1e6))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
