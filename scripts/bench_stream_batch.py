#!/usr/bin/env python3
"""Streamed batch decompress (lep_decompress_batch_stream): 1, 8 and 64 generated 4K files at bands of 1, 4 and 16 MCU rows -- the time
to every file's first scan byte (median and worst over the files), the wall time beside lep_decompress_batch on the same files in the
same process, and LEP_STREAM_PACK=1 against 0 (a fresh codec each: the switch is read when the codec is made), alternating runs.
One JSON line per measurement.
--slice-bytes N: the measured files are not whole files but what a block store holds of them -- every generated file (--quality, 97 for
files of several MiB) cut into consecutive slices of N bytes with lep_compress_slice: the first a 'Z' file cut inside its scan, the others
'Y' files, all but the last cut as well.  --files then counts slices; the pack comparison is left out.
usage: python scripts/bench_stream_batch.py [--files 1,8,64] [--bands 1,4,16] [--runs 5] [--width 3840 --height 2160]
                                            [--slice-bytes 4194304 --quality 97]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def head_bytes(lep):
    """bytes a streamed file sends in front of its scan (a slice's may be none)"""
    from lepton_amd import abi
    from lepton_amd.codec import LepFile

    f = LepFile(lep)
    img, segs = abi.HuffImage(), (abi.HuffSegment * abi.MAX_SEGMENTS)()
    nseg, ok = C.c_int(0), C.c_int(0)
    data, n = C.c_void_p(), C.c_size_t(0)
    assert abi.lib().lep_file_recode_plan(f.handle, C.byref(img), segs, C.byref(nseg), C.byref(ok)) == 0 and ok.value
    assert abi.lib().lep_file_recode_head(f.handle, C.byref(data), C.byref(n)) == 0
    return n.value


def stream_once(codec, leps, band, heads=None):
    """(wall seconds, seconds to each file's first piece that holds scan bytes, stats); heads: bytes in front of each file's scan
    (None: piece 1 is the header)"""
    from lepton_amd import abi

    n = len(leps)
    ins = (abi.Bytes * n)()
    keep = [C.create_string_buffer(b, len(b)) for b in leps]
    for i, b in enumerate(keep):
        ins[i].data, ins[i].len, ins[i].cap = C.cast(b, C.c_void_p).value, len(leps[i]), len(leps[i])
    calls = [0] * n
    first = [None] * n
    total = [0] * n
    t0 = time.perf_counter()

    def sink(_user, i, _data, k):
        calls[i] += 1
        total[i] += k
        if first[i] is None and (calls[i] == 2 if heads is None else total[i] > heads[i]):    # (piece 1 is the header; a file that is not streamed has one piece, counted below)
            first[i] = time.perf_counter() - t0
        return 0

    status = (C.c_int32 * n)()
    stats = abi.BatchStreamStats()
    opt = abi.BatchOptions()
    rc = abi.lib().lep_decompress_batch_stream(codec.handle, ins, n, band, abi.BATCH_SINK_FN(sink), None, status, C.byref(opt), C.byref(stats))
    wall = time.perf_counter() - t0
    assert rc == 0 and not any(status), (rc, list(status))
    return wall, [f if f is not None else wall for f in first], {k: getattr(stats, k) for k, _ in abi.BatchStreamStats._fields_}, total


def abi_streams(lep):
    from lepton_amd import abi

    return abi.lib().lep_file_streams_in_session(lep, len(lep)) == 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", default="1,8,64")
    ap.add_argument("--bands", default="1,4,16")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--unique", type=int, default=8)
    ap.add_argument("--slice-bytes", type=int, default=0)
    ap.add_argument("--quality", type=int, default=90)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from lepton_amd import corpus
    from lepton_amd.codec import GpuCodec

    counts = [int(x) for x in args.files.split(",")]
    bands = [int(x) for x in args.bands.split(",")]
    codec = GpuCodec(0)
    nu = min(args.unique, max(counts))
    jpgs = corpus.make_corpus(nu, args.width, args.height, 10000, quality=args.quality)
    heads = None
    if args.slice_bytes:
        cuts = [(j, k, min(k + args.slice_bytes, len(j))) for j in jpgs for k in range(0, len(j), args.slice_bytes)]
        uniq, st, _ = codec.compress_batch([j for j, _, _ in cuts], slices=[(a, 0 if b == len(j) else b) for j, a, b in cuts])
        jpgs = [j[a:b] for j, a, b in cuts]
        nu = len(cuts)
        assert not any(st) and all(abi_streams(u) for u in uniq)
        heads = [head_bytes(u) for u in uniq]
    else:
        uniq, st, _ = codec.compress_batch(jpgs)
    assert not any(st)
    for n in counts:
        leps = [uniq[i % nu] for i in range(n)]
        want = [jpgs[i % nu] for i in range(n)]
        hd = [heads[i % nu] for i in range(n)] if heads else None
        back, st, _ = codec.decompress_batch(leps)    # warm: kernel images, staging
        assert not any(st) and back == want
        whole = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            codec.decompress_batch(leps)
            whole.append(time.perf_counter() - t0)
        for band in bands:
            stream_once(codec, leps, band, hd)    # warm
            walls, firsts, stats = [], [], None
            for _ in range(args.runs):
                wall, first, stats, total = stream_once(codec, leps, band, hd)
                assert total == [len(j) for j in want] and stats["files_streamed"] == n
                walls.append(wall)
                firsts.append(first)
            med = statistics.median
            print(json.dumps({
                "files": n, "slice_bytes": args.slice_bytes, "band_mcu_rows": band, "runs": args.runs, "jpeg_mb": round(sum(map(len, want)) / 1e6, 2),
                "first_scan_byte_ms_median_over_files": round(1e3 * med([med(f) for f in firsts]), 2),
                "first_scan_byte_ms_worst_file": round(1e3 * med([max(f) for f in firsts]), 2),
                "stream_wall_ms": round(1e3 * med(walls), 2), "stream_wall_ms_runs": [round(1e3 * w, 1) for w in walls],
                "batch_wall_ms": round(1e3 * med(whole), 2), "batch_wall_ms_runs": [round(1e3 * w, 1) for w in whole],
                "sessions": stats["sessions"], "advances": stats["advances"], "writer_launches": stats["writer_launches"],
                "scan_bytes_down": stats["scan_bytes_down"], "frame_bytes_down": stats["frame_bytes_down"],
                "files_first_scan_byte_before_last_advance": stats["files_first_scan_byte_before_last_advance"]}), flush=True)
    if args.slice_bytes:
        return
    # the pack pass against one copy per segment: alternating runs, a fresh codec per setting
    n, band = max(counts), bands[0]
    leps = [uniq[i % nu] for i in range(n)]
    codecs = {}
    for setting in ("1", "0"):
        os.environ["LEP_STREAM_PACK"] = setting
        codecs[setting] = GpuCodec(0)
        stream_once(codecs[setting], leps, band)    # warm
    os.environ.pop("LEP_STREAM_PACK", None)
    res = {"1": [], "0": []}
    for _ in range(args.runs):
        for setting in ("1", "0"):
            res[setting].append(stream_once(codecs[setting], leps, band)[0])
    print(json.dumps({"files": n, "band_mcu_rows": band, "pack_wall_ms_runs": [round(1e3 * w, 1) for w in res["1"]],
                      "copy_per_segment_wall_ms_runs": [round(1e3 * w, 1) for w in res["0"]],
                      "pack_wall_ms": round(1e3 * statistics.median(res["1"]), 2), "copy_per_segment_wall_ms": round(1e3 * statistics.median(res["0"]), 2)}), flush=True)


if __name__ == "__main__":
    main()
