#!/usr/bin/env python3
"""Byte-range reads against the whole decode: 4K files of bench.py's generator (lepton_amd.corpus.make_corpus; nothing is downloaded),
per file four ranges -- the first 64 KB, 64 KB in the middle of thread segment 3, the last 64 KB, the header only -- each run ALONE
(lep_decompress_range, one file) and as 64 REQUESTS IN ONE CALL (lep_decompress_batch_ranges, 64 files).  The baseline is
lep_decompress_batch on the same files -- one file, and 64 files -- in ANOTHER BUILD of the library (LEP_LIB_PATH=<the parent commit's
liblepton_mi355x.so>), which has no range call; the builds are alternated in one visit by running this script once per build and round
(one JSON line per run), and `--summarize FILE...` turns the lines of all runs into the tables: medians and ranges over the rounds, and
for every range case the call's counters (advances, rows decoded of rows begun, bytes down).

usage: python scripts/bench_ranges.py [--files 64] [--distinct 8] [--repeats 5] [--band 0] [--label NAME]
       python scripts/bench_ranges.py --summarize runs/ranges_*.jsonl"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KB64 = 65536


def timed(fn, repeats):
    fn()   # warm
    secs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        secs.append(time.perf_counter() - t0)
    return {"median_ms": round(statistics.median(secs) * 1e3, 2), "min_ms": round(min(secs) * 1e3, 2), "max_ms": round(max(secs) * 1e3, 2)}


def cases_of(plan):
    """the four ranges of a file, from its range plan: (name, first, length)"""
    q = min(3, plan.nseg - 1)
    return [("first_64k", 0, KB64),
            ("mid_segment_3_64k", plan.seg_first[q] + max(0, (plan.seg_len[q] - KB64) // 2), KB64),
            ("last_64k", max(0, plan.jpeg_size - KB64), 0),
            ("header_only", 0, plan.head_len)]


def run(a):
    import ctypes as C

    from lepton_amd import abi, corpus
    from lepton_amd.codec import GpuCodec

    L = abi.lib()
    ranged = hasattr(L, "lep_decompress_batch_ranges")
    codec = GpuCodec(0)
    uniq = corpus.make_corpus(a.distinct, a.width, a.height, 10000)
    leps_u, st, _ = codec.compress_batch(uniq)
    assert st == [0] * len(uniq)
    leps = [leps_u[i % len(leps_u)] for i in range(a.files)]
    out = {"label": a.label, "library": abi.LIB_PATH, "files": a.files, "distinct": a.distinct, "size": [a.width, a.height],
           "jpeg_bytes_one": len(uniq[0]), "repeats": a.repeats, "band": a.band, "cases": {}}
    # the whole decode, in either build: one file, and all of them in one call
    back, st, _ = codec.decompress_batch(leps)
    assert st == [0] * len(leps) and back[0] == uniq[0]
    out["whole_decode_one_file"] = timed(lambda: codec.decompress_batch(leps[:1]), a.repeats)
    out["whole_decode_%d_files" % a.files] = timed(lambda: codec.decompress_batch(leps), a.repeats)
    if ranged:
        plans = []
        for lep in leps_u:
            rp = abi.RangePlan()
            assert L.lep_file_range_plan(lep, len(lep), 0, 0, C.byref(rp)) == 0 and rp.in_session == 1
            plans.append(rp)
        out["segments_per_file"] = plans[0].nseg
        for k, name in enumerate(n for n, _, _ in cases_of(plans[0])):
            one = cases_of(plans[0])[k][1:]
            many = [cases_of(plans[i % len(plans)])[k][1:] for i in range(a.files)]
            got, st, counters = codec.decompress_batch_ranges(leps[:1], [one], a.band)
            assert st == [0] and got[0] == (uniq[0][one[0]:one[0] + one[1]] if one[1] else uniq[0][one[0]:]), name
            got, st, counters_many = codec.decompress_batch_ranges(leps, many, a.band)
            assert st == [0] * len(leps)
            for i in (0, len(leps) - 1):
                f, n = many[i]
                assert got[i] == (uniq[i % len(uniq)][f:f + n] if n else uniq[i % len(uniq)][f:]), (name, i)
            keep = ("files_ranged", "files_whole", "files_no_decode", "sessions", "advances", "writer_launches", "segments_begun", "segments_retired",
                    "mcu_rows_begun", "mcu_rows_decoded", "scan_bytes_down", "frame_bytes_down")
            out["cases"][name] = {
                "one_file": dict(timed(lambda: codec.decompress_range(leps[0], one[0], one[1]), a.repeats), **{c: counters[c] for c in keep}),
                "%d_files" % a.files: dict(timed(lambda: codec.decompress_batch_ranges(leps, many, a.band), a.repeats), **{c: counters_many[c] for c in keep})}
    codec.close()
    print(json.dumps(out), flush=True)


def spread(values):
    return "%8.2f  [%8.2f .. %8.2f]" % (statistics.median(values), min(values), max(values))


def summarize(paths):
    runs = [json.loads(line) for p in paths for line in open(p) if line.startswith("{")]
    labels = sorted({r["label"] for r in runs})
    print("byte-range reads against the whole decode: medians of the runs' medians [least .. most], ms; %d runs" % len(runs))
    for r in runs[:1]:
        print("corpus: %d files of %dx%d (%d distinct, %d bytes the first), %d repeats per run, band %d (0: 1, 2, 4, ... MCU rows)" % (
            r["files"], r["size"][0], r["size"][1], r["distinct"], r["jpeg_bytes_one"], r["repeats"], r["band"]))
    for label in labels:
        mine = [r for r in runs if r["label"] == label]
        print("\n== %s (%d runs) %s" % (label, len(mine), mine[0]["library"]))
        for key in sorted(k for k in mine[0] if k.startswith("whole_decode")):
            print("  %-34s %s" % (key, spread([r[key]["median_ms"] for r in mine])))
        for name in mine[0]["cases"]:
            for form in mine[0]["cases"][name]:
                c = mine[0]["cases"][name][form]
                print("  %-22s %-11s %s   advances %d, rows %d of %d, segments %d (retired %d), scan bytes down %d, frames %d, no decode %d" % (
                    name, form, spread([r["cases"][name][form]["median_ms"] for r in mine]), c["advances"], c["mcu_rows_decoded"], c["mcu_rows_begun"],
                    c["segments_begun"], c["segments_retired"], c["scan_bytes_down"], c["frame_bytes_down"], c["files_no_decode"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--band", type=int, default=0)
    ap.add_argument("--label", default=os.environ.get("LEP_LIB_PATH") and "parent (LEP_LIB_PATH)" or "this build")
    ap.add_argument("--summarize", nargs="+", metavar="FILE")
    a = ap.parse_args()
    if a.summarize:
        summarize(a.summarize)
    else:
        run(a)


if __name__ == "__main__":
    main()
