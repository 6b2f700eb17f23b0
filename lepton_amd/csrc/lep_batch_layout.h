// lep_batch_layout.h -- the layout arithmetic and the launch order of the batch pipelines (lep_batch.hip): where a chunk's scans, restart
// tables, reference copies and row records lie in the scan arena, how outputs get their slots, how large a stream slot is, when an arena
// comes down in one copy, whether the GPU's answer for a re-coded file stands, and which stream and workspace set a decompress chunk's
// launch takes.  Host code only (the C ABI header and the standard library): the pipeline reserves, fills, uploads and launches what these
// say and decides nothing, and tests/emu/batch_layout_probe.cc holds every rule against hand-computed answers without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/lepton_mi355x.h"

namespace lepbatch {

inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

// restart positions (uint32 offsets) sit behind a scan's room, padded to 16 bytes
inline size_t restart_table_bytes(size_t n) { return align16(n * 4); }

// ---- compress: the scan arena (pinned -> device) and the row records ---------------------------------------------------------------
enum Route : uint8_t { kHost = 0, kSequential = 1, kProgressive = 2 };   // host parser / one sequential scan on the GPU / progressive on the GPU

struct ScanPlace {            // one scan of a progressive file
    uint32_t scan_len = 0;    // in: un-stuffed bytes
    size_t restarts = 0;      // in: restart positions behind the scan's slot (0 without LEP_HUFFDEC_RST_TABLE)
    uint32_t ref_len = 0;     // in, verify: the scan's bytes as they stand in the file
    size_t off = 0, table_off = 0, ref_off = 0;   // out
};
struct ScanArenaImage {       // one live image of a chunk
    Route route = kHost;
    uint32_t scan_len = 0;    // in, sequential: un-stuffed bytes, restart positions (0 without the flag), MCU rows,
    size_t restarts = 0;
    int32_t mcuv = 0;
    uint32_t ref_len = 0;     // ... and under verify the whole scan as it stands in the file (0: none)
    std::vector<ScanPlace> scans;   // in / out, progressive
    int32_t prow_need = 0;    // in, progressive: row records
    size_t scan_off = 0, table_off = 0, ref_off = 0;   // out, sequential
    size_t row_off = 0;       // out: first row record
};
struct ScanArenaTotals { size_t scan_total = 0, rows_total = 0; };

// Placement order: all sequential images in chunk order, all progressive images scan by scan, the progressive reference copies, the
// sequential reference copies; row records: sequential images (mcuv + 1 each), then progressive (prow_need each).
// Rec: ScanArenaImage or a record derived from it.
template <class Rec>
ScanArenaTotals lay_out_scan_arena(Rec* recs, size_t n, bool verify) {
    ScanArenaTotals t;
    for (size_t k = 0; k < n; ++k) {
        ScanArenaImage& im = recs[k];
        if (im.route != kSequential) continue;
        im.scan_off = t.scan_total; t.scan_total += LEP_HUFFDEC_SCAN_ROOM(im.scan_len);
        im.table_off = t.scan_total; t.scan_total += restart_table_bytes(im.restarts);
        im.row_off = t.rows_total; t.rows_total += (size_t)im.mcuv + 1;
    }
    for (size_t k = 0; k < n; ++k) {
        ScanArenaImage& im = recs[k];
        if (im.route != kProgressive) continue;
        for (ScanPlace& sc : im.scans) {   // every scan in its own aligned, zero-padded slot
            sc.off = t.scan_total; t.scan_total += LEP_HUFFPROGDEC_SCAN_ROOM(sc.scan_len);
            sc.table_off = t.scan_total; t.scan_total += restart_table_bytes(sc.restarts);
        }
        im.row_off = t.rows_total; t.rows_total += (size_t)im.prow_need;
    }
    if (!verify) return t;
    for (size_t k = 0; k < n; ++k) {
        ScanArenaImage& im = recs[k];
        if (im.route == kProgressive)
            for (ScanPlace& sc : im.scans) { sc.ref_off = t.scan_total; t.scan_total += align16(sc.ref_len); }
    }
    for (size_t k = 0; k < n; ++k) {
        ScanArenaImage& im = recs[k];
        if (im.route == kSequential && im.ref_len) { im.ref_off = t.scan_total; t.scan_total += align16(im.ref_len); }
    }
    return t;
}

// ---- output arenas: give an output its slot ------------------------------------------------------------------------------------------
struct OutputArena {
    size_t bytes = 0, corr_words = 0;
    size_t place(size_t cap) { const size_t off = bytes; bytes += align16(cap); return off; }          // 16-byte aligned cumulative offset
    size_t place_corr(size_t words) { const size_t off = corr_words; corr_words += words; return off; }   // cumulative correction words
};

// round-trip check: an output longer than its reference by 64 bytes is a mismatch anyway
inline uint32_t verify_out_cap(uint32_t out_cap, uint32_t ref_len) { return (uint32_t)std::min<size_t>(out_cap, (size_t)ref_len + 64); }

// decompress scan arena: segment 0 is only bounded by the file, so it gets what the later segments leave, plus slack
struct RecodeSlot { uint64_t off; uint32_t slot, bound; };   // arena offset, bytes reserved, the segment's real byte bound
inline void place_recode_segments(const uint32_t* caps, int ns, OutputArena* arena, RecodeSlot* out) {
    size_t later = 0;
    for (int q = 1; q < ns; ++q) later += caps[q];
    for (int q = 0; q < ns; ++q) {
        size_t slot = caps[q];
        if (q == 0) slot = std::min<size_t>(caps[0], (caps[0] > later ? caps[0] - later : 0) + 8192);
        out[q].bound = caps[q];
        out[q].slot = (uint32_t)slot;
        out[q].off = arena->place(slot);
    }
}

// A thread segment's room in the stream arena.  Segments are cut by equal JPEG bytes, not blocks, so the segment's own scan bytes (+ 25 %)
// are the measure; the per-block term covers progressive files, whose hand-offs only count the first scan (baseline files take the byte
// measure alone: the per-block term made a 4K segment's slot 1 MB for 0.2 MB of stream, and the whole arena comes down in one copy).
inline size_t stream_slot_bytes(size_t segment_size, size_t frame_blocks, int nseg, bool progressive) {
    const size_t by_bytes = segment_size + segment_size / 4, by_blocks = progressive ? frame_blocks * 40 / (size_t)nseg : 0;
    return (std::max(by_bytes, by_blocks) + 65536 + 255) & ~(size_t)255;
}

// bring an arena down in one copy of its extent unless it is mostly slack
inline bool download_whole(size_t extent, size_t live_bytes) { return extent <= 3 * live_bytes + ((size_t)1 << 20); }

// Does the GPU's answer for a re-coded file stand?  A segment that filled its reserved slot may have been cut short; a truncated file's
// segments are the file's bytes only if the encoder stopped at the cut in the LAST thread with that thread's byte bound reached
// (lep_huff_simt.h code_mcus, recode_finish) -- otherwise the host re-coder takes the file.  All arrays: the file's ns segments.
inline bool gpu_answer_stands(const uint32_t* slens, const uint32_t* hslot, const uint32_t* hbound, const lep_huff_end* ends, int ns) {
    for (int q = 0; q < ns; ++q) {
        if (slens[q] >= hslot[q] && hslot[q] < hbound[q]) return false;
        if (ends[q].pad & 2) return false;
        if ((ends[q].pad & 1) && (q + 1 != ns || ends[q].attempted < hbound[q])) return false;
    }
    return true;
}

// ---- decompress: which stream and workspace set a chunk's launch takes -------------------------------------------------------------
// Consecutive chunks' decode kernels go to TWO streams (A, B) and the codec's two workspace sets where that pays: behind a ragged chunk
// (segments whose block counts differ by more than 1.5x, or fewer segments than fill the chip) the next launch goes BESIDE it, on the
// other stream and set; behind a chunk of equal segments it waits in stream order on the same stream and set.
struct LaunchPlace {
    int stream;            // 0 = A, 1 = B
    int set;               // workspace set
    bool beside;           // beside the previous launch (other stream), not behind it
    bool ragged;           // this chunk leaves a tail
    bool expect_company;   // the decode launch shares the chip with a neighbour
    int prev_slot;         // the slot of the launch in front (-1: none)
};
struct LaunchOrder {
    int prev_stream = -1, prev_slot = -1, prev_set = 0;   // -1: nothing launched yet
    bool prev_ragged = false;
    // lo / hi: fewest / most blocks of a thread segment of the chunk; dec_overlap: -1 automatic, 0 never, 1 always; scan_separate: the
    // scan encoders have the second stream to themselves (every launch on A, set 0); whole_call: the chunk is all of the call
    LaunchPlace step(int64_t lo, int64_t hi, int nseg, int dec_overlap, bool scan_separate, bool whole_call, int slot) {
        if (scan_separate) dec_overlap = 0;
        LaunchPlace p;
        p.ragged = hi * 2 > lo * 3 || nseg < 6144;
        const bool first = prev_stream < 0;
        p.beside = !first && (dec_overlap == 1 || (dec_overlap < 0 && prev_ragged));
        // the second workspace set (its own 3 MB of model per segment) only where two launches are in flight; launches in stream order share one
        p.set = first ? 0 : (p.beside ? prev_set ^ 1 : prev_set);
        p.stream = first ? 0 : (p.beside ? prev_stream ^ 1 : prev_stream);
        p.expect_company = dec_overlap != 0 && (p.beside || p.ragged) && !whole_call;   // (a call of one chunk has no neighbour)
        p.prev_slot = prev_slot;
        prev_stream = p.stream; prev_set = p.set; prev_ragged = p.ragged; prev_slot = slot;
        return p;
    }
};

// ---- descriptors ----------------------------------------------------------------------------------------------------------------------
// Point a descriptor's component pointers into the frame at `frame`: component c takes blocks_of(c) blocks of 128 bytes behind the ones in
// front of it; the entries behind ncomp are null.
template <class Ptr, size_t N, class BlocksOf>
inline void point_components(Ptr (&blocks)[N], int ncomp, char* frame, BlocksOf blocks_of) {
    size_t off = 0;
    for (int c = 0; c < (int)N; ++c) {
        blocks[c] = c < ncomp ? (Ptr)(frame + off) : nullptr;
        if (c < ncomp) off += (size_t)blocks_of(c) * 128;
    }
}
inline size_t desc_blocks(const lep_image_desc& d, int c) { return (size_t)d.width_blocks[c] * d.height_blocks[c]; }

}  // namespace lepbatch
