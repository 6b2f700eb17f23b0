// prog_cut_driver.h -- TEST ONLY: progressive files that END INSIDE A SCAN on the scan kernels, as the batch pipelines run them.  Decode: every
// scan of the file in a slot of its own (LEP_HUFFPROGDEC_SCAN_ROOM) whose room, and everything behind it, is 0xFF -- the window decoder must
// take the bits behind the data's last for zeros by position, not from what the slot holds -- then the launch code's plan
// (lep_scan_decode_plan.h through scan_dec_driver.h), the final records of the scans it declines marked as the launch code marks them.
// Write: the lane-per-unit scan writer (lep_huffprog_simt.h through prog_simt_driver.h) over the frame of such a file, with the clear of the
// lazy tail the batch pipeline puts between the decode and the scan launch.
// Included by prog_cut_emu.cc, which the tests build as a library of its own.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "scan_dec_driver.h"
#include "prog_simt_driver.h"

// scans[i].t.scan: the scan's OFFSET in `raw` (the file's un-stuffed scan bytes), as lep_jpeg_open_gpu_progressive leaves it; blocks: the
// caller's zeroed frame.  win / pipelined: the launch object's knobs.  misalign: the cut scan's slot one byte off (prog_win_takes refuses it).
// declined_out: scans the plan sent to no kernel; win_taken: scans the window form decoded.
inline int emu_prog_cut_decode(const lephuff::ProgDecScan* scans_in, int nscan, const uint8_t* raw, size_t raw_len, bool win, bool pipelined, bool misalign,
                               lephuff::HuffDecRow* rows, int32_t* win_taken, int32_t* declined_out) {
    std::vector<lephuff::ProgDecScan> scans(scans_in, scans_in + nscan);
    size_t total = 0;
    std::vector<size_t> at((size_t)nscan);
    for (int i = 0; i < nscan; ++i) { at[(size_t)i] = total; total += (((size_t)scans[(size_t)i].t.scan_len) + 80 + 15) & ~(size_t)15; }
    void* mem = nullptr;
    if (posix_memalign(&mem, 64, total + 512)) return -2;
    uint8_t* arena = static_cast<uint8_t*>(mem);
    memset(arena, 0xFF, total + 512);
    for (int i = 0; i < nscan; ++i) {
        lephuff::ProgDecScan& sc = scans[(size_t)i];
        const size_t off = (size_t)reinterpret_cast<uintptr_t>(sc.t.scan);
        if (off + sc.t.scan_len > raw_len) { free(mem); return -2; }
        uint8_t* slot = arena + at[(size_t)i] + ((misalign && (sc.t.flags & lephuff::kHuffDecEarlyEof)) ? 1 : 0);
        memcpy(slot, raw + off, sc.t.scan_len);
        sc.t.scan = slot;
    }
    lephuff::ProgDecOptions o;
    o.lanes = true; o.win = win; o.rst = true; o.pipeline = pipelined; o.pipeline_max = 1 << 20; o.split = false;
    lephuff::ProgDecPlan plan;
    if (lephuff::prog_dec_plan(scans.data(), nscan, o, &plan)) { free(mem); return -1; }
    for (uint64_t r : plan.declined) memset(rows + r, lephuff::kProgDecDeclinedFill, sizeof rows[0]);
    if (declined_out) *declined_out = (int32_t)plan.declined.size();
    const int rc = emu_prog_dec_drive(scans.data(), nscan, o, rows, nullptr, win_taken);
    free(mem);
    return rc;
}

// The scans of a cut file written again from its frame (lep_file_recode_plan_progressive_cut's image and descriptors, out_off / corr_off placed by
// the caller).  nsegs == 1: the blocks at or behind coded_blocks[c] are cleared first, as lep_batch.hip clears them on the device -- the
// reference's re-coder reads zeros there even where the stream coded a row's first block.  taken[i] as emu_prog_simt_drive's.
inline int emu_prog_cut_write(const lep_huffprog_image* img, const lep_huffprog_scan* scans, int nscan, int nsegs, const int32_t* coded_blocks, uint8_t* out, uint32_t* corr,
                              uint32_t* out_len, int32_t* taken, int32_t* guards_intact) {
    const lephuff::ProgImage* im = reinterpret_cast<const lephuff::ProgImage*>(img);
    if (nsegs == 1)
        for (int c = 0; c < im->ncomp && c < 4; ++c) {
            const int64_t all = (int64_t)im->bch[c] * im->bcv[c], coded = coded_blocks[c];
            if (coded >= 0 && coded < all) memset(const_cast<int16_t*>(im->blocks[c]) + coded * 64, 0, (size_t)(all - coded) * 128);
        }
    return emu_prog_simt_drive(img, scans, nscan, out, corr, out_len, taken, 0, true, nullptr, guards_intact);
}
