#!/usr/bin/env python3
"""Slices through the batch pipeline: `--slices` slices of `--slice-mb` MiB (S = 0, slice, 2 x slice, ...; T = S + slice) cut from 4K
files, through lep_compress_batch_slices / lep_decompress_batch, against a loop of lep_compress_slice / lep_decompress over the same
slices -- the per-file path is what a library without the batch entry point offers (LEP_LIB_PATH names such a build for an A/B run;
it then runs the loop alone).  Host memory to host memory, PCIe included.  Prints one JSON line.
usage: python scripts/bench_slices.py [--slices 1024] [--slice-mb 4] [--unique 16] [--loop-slices 64] [--verify]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slices", type=int, default=1024)
    ap.add_argument("--slice-mb", type=float, default=4.0, help="slice size in MiB; must lie below the corpus files' size (the synthetic 4K corpus: pass 0.5)")
    ap.add_argument("--unique", type=int, default=16)
    ap.add_argument("--loop-slices", type=int, default=64, help="slices the per-file loop is timed on (it is slow: the rate is per slice)")
    ap.add_argument("--verify", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    from lepton_amd import abi, corpus
    from lepton_amd.codec import GpuCodec, LeptonError

    codec = GpuCodec(0)
    uniq = corpus.make_corpus(max(1, args.unique), 3840, 2160, 10000)
    step = int(args.slice_mb * (1 << 20))
    pairs = []
    while len(pairs) < args.slices:
        for f in uniq:
            for s in range(0, len(f), step):
                pairs.append((f, s, min(s + step, len(f))))
    pairs = pairs[:args.slices]
    # (a file shorter than one slice would give the pair (0, len): a whole file, no slice at all)
    inner = sum(1 for _, s, _ in pairs if s > 0)
    assert inner * 2 >= len(pairs), "only %d of %d pairs start inside their file (files of %d .. %d bytes): choose --slice-mb below the file size" % (
        inner, len(pairs), min(map(len, uniq)), max(map(len, uniq)))
    mb = sum(t - s for _, s, t in pairs) / 1e6
    out = {"workload": "%d slices of %.1f MiB from %d 4K files" % (len(pairs), args.slice_mb, len(uniq)), "slice_MB": round(mb, 1)}
    # the per-file loop
    loop = pairs[:max(1, min(args.loop_slices, len(pairs)))]
    t0 = time.perf_counter()
    leps, codes = [], []
    for f, s, t in loop:
        try:
            leps.append(codec.compress_slice(f, s, t)); codes.append(0)
        except LeptonError as e:
            leps.append(None); codes.append(e.code)
    t1 = time.perf_counter()
    back = [codec.decompress(x) for x in leps if x is not None]
    t2 = time.perf_counter()
    assert back == [f[s:t] for (f, s, t), x in zip(loop, leps) if x is not None]
    lmb = sum(t - s for _, s, t in loop) / 1e6
    out["loop"] = {"slices": len(loop), "compress_MBps": round(lmb / (t1 - t0), 1), "decompress_MBps": round(lmb / (t2 - t1), 1), "refused": sum(1 for c in codes if c)}
    if hasattr(abi.lib(), "lep_compress_batch_slices"):
        files, sl = [p[0] for p in pairs], [(p[1], p[2]) for p in pairs]
        codec.compress_batch(files[:64], verify=args.verify, slices=sl[:64])            # warm: kernel images, staging
        t0 = time.perf_counter()
        bl, st, cs = codec.compress_batch(files, verify=args.verify, slices=sl)
        t1 = time.perf_counter()
        assert bl[:len(loop)] == leps and st[:len(loop)] == codes, "the batch differs from the per-file path"
        good = [x for x in bl if x is not None]
        bj, st2, ds = codec.decompress_batch(good)
        t2 = time.perf_counter()
        assert not any(st2) and bj == [f[s:t] for (f, s, t), x in zip(pairs, bl) if x is not None]
        out["batch"] = {"compress_MBps": round(mb / (t1 - t0), 1), "decompress_MBps": round(mb / (t2 - t1), 1), "refused": sum(1 for c in st if c),
                        "gpu_huffman_files": [cs["gpu_huffman_files"], ds["gpu_huffman_files"]], "redone_files": cs["redone_files"], "verify": bool(args.verify)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
