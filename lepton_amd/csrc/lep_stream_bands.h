// lep_stream_bands.h -- host only: the bookkeeping of a decode session whose completed MCU rows are written by the scan writer band after
// band (lep_decompress_batch_stream, lep_batch_stream.cc; stepped on the CPU by tests/emu/stream_bands_emu.cc and stream_layouts_emu.cc).  Per thread segment:
// which rows a band added, the state the band's writer starts from (the end state of the band before, the file's hand-off for the first),
// where in the segment's slot its bytes go; per file: which bytes may go out (a segment's only when every segment in front of it is
// complete), and whether what went out is the front of the finished file.  Nothing here touches a device or a socket.
// Rows are the PLAN's rows throughout (lep_huff_segment.mcu_row0 / mcu_row1): MCU rows of an interleaved file, block rows of a one-component
// file (lep_huff_image.interleaved, recode_prepare) -- RowUnits converts the decoder's block-row counts and the band height into them.
// A -startbyte / -trunc slice ('Y') has no rule of its own here: its head is the prefix garbage, its first segment is seeded with the
// overhang of the row it starts in, its bounds are the slice's -- all of it the plan's (recode_prepare), so it is stepped like a whole file.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/lepton_mi355x.h"

namespace lepbands {

struct Segment {
    int file = 0;                  // the session's file this segment belongs to
    int row0 = 0, row1 = 0;        // its MCU rows (lep_huff_segment.mcu_row0 / mcu_row1 of the file's plan)
    int coded = 0;                 // rows below this one are written
    uint32_t overhang = 0;         // what the next band's writer starts from
    int16_t last_dc[4] = {0, 0, 0, 0};
    uint64_t slot_off = 0;         // the segment's slot in the scan arena
    uint32_t slot_cap = 0;         // ... its size
    uint32_t bound = 0;            // the segment's byte bound itself (a front segment's slot may be smaller: place_recode_segments)
    bool last = false;             // the file's last segment: the one a cut inside the scan may end (band_written)
    uint32_t written = 0;          // bytes of the slot that are written
    bool stopped = false;          // its decode failed: nothing more is written
    std::vector<uint8_t> bytes;    // host copy of the written bytes (what recode_finish is given)
    size_t given = 0;              // ... of which the sink has this many
    lep_huff_end end;              // end state of the last band
    Segment() { memset(&end, 0, sizeof end); }
    bool complete() const { return coded >= row1; }
};

struct File {
    int seg0 = 0, nseg = 0;        // its segments in the session's list
    int front = 0;                 // first segment (0 .. nseg) whose bytes are not all out
    bool failed = false;           // a segment's decode failed: nothing more goes out
    int32_t fail_status = 0;
    bool declined = false;         // the writer's byte bound was outgrown (or it refused the segment): the host re-coder finishes the file
    bool gone = false;             // the sink said its receiver is gone
    uint64_t sunk = 0;             // bytes the sink has, header included
    bool scan_byte_out = false;
    bool writes() const { return !failed && !declined && !gone; }
};

// planned.out_cap is the slot's size; bound: the plan's byte bound where the slot was given another size (0: the slot's)
inline void start_segment(Segment* s, int file, const lep_huff_segment& planned, uint64_t slot_off, bool last_of_file = false, uint32_t bound = 0) {
    s->file = file;
    s->last = last_of_file; s->bound = bound ? bound : planned.out_cap;
    s->row0 = planned.mcu_row0; s->row1 = std::max(planned.mcu_row0, planned.mcu_row1); s->coded = s->row0;
    s->overhang = planned.overhang;
    memcpy(s->last_dc, planned.last_dc, sizeof s->last_dc);
    s->slot_off = slot_off; s->slot_cap = planned.out_cap;
    s->end.overhang_byte = (uint8_t)(planned.overhang & 255u); s->end.num_overhang_bits = (uint8_t)((planned.overhang >> 8) & 255u);
    memcpy(s->end.last_dc, planned.last_dc, sizeof s->end.last_dc);
}

// Block rows of every component per MCU row, from the geometry the decoder's rows_done counts in (lep_image_desc).
inline void block_rows_per_mcu_row(const lep_image_desc& d, int* vs) {
    for (int c = 0; c < d.ncomp && c < LEP_MAX_COMPONENTS; ++c) vs[c] = std::max(d.height_blocks[c] / std::max(d.mcu_rows, 1), 1);
}

// The plan's row unit against the decoder's: vs[c] = block rows of component c per planned row, per_mcu_row = planned rows per MCU row
// (what one band_mcu_rows of an advance adds).  Interleaved: planned rows ARE MCU rows -- the geometry's ratio, 1.  One component: the
// writer's plan is nch x ncv MCUs of one block and its segments are in block rows (clipped to ncv: rows that only pad the frame to whole
// MCUs are never written, so the last MCU row may hold fewer), while rows_done[0] counts frame block rows -- 1, and the frame's block
// rows per MCU row (the hand-offs' luma_mul).
struct RowUnits { int vs[LEP_MAX_COMPONENTS] = {1, 1, 1}; int per_mcu_row = 1; };
template <class PlanImage>   // lep_huff_image, or recode_prepare's RecodeImage of the same layout
inline RowUnits row_units(const lep_image_desc& d, const PlanImage& plan) {
    RowUnits u;
    if (plan.ncomp == 1) u.per_mcu_row = std::max(d.height_blocks[0] / std::max(d.mcu_rows, 1), 1);
    else block_rows_per_mcu_row(d, u.vs);
    return u;
}

// The planned row up to which segment s is in the frame after an advance: every component's block rows below rows_done[c] are there, a
// finished segment is there to its end.  vs[c] = block rows of component c per planned row (RowUnits::vs).
inline int complete_row(const Segment& s, const lep_decode_progress& p, const int* vs, int ncomp) {
    if (p.status == 0) return s.row1;
    int complete = s.row1;
    for (int c = 0; c < ncomp; ++c) complete = std::min(complete, p.rows_done[c] / std::max(vs[c], 1));
    return std::max(complete, s.coded);
}

// The writer's work for the rows [coded, complete): false = none.  `planned` supplies image index and whatever else the plan set.
inline bool band_segment(const Segment& s, int complete, int image, lep_huff_segment* out) {
    if (s.stopped || complete <= s.coded) return false;
    memset(out, 0, sizeof *out);
    out->image = image;
    out->mcu_row0 = s.coded; out->mcu_row1 = std::min(complete, s.row1);
    out->overhang = s.overhang;
    memcpy(out->last_dc, s.last_dc, sizeof out->last_dc);
    out->out_off = s.slot_off + s.written;
    out->out_cap = s.slot_cap - s.written;
    return true;
}

// What the band's writer answered: len bytes at `data` (the host copy of slot_off + written ...), its end state.  false = the band did
// not fit what was left of the slot, or the writer stopped of its own accord: the file is the host re-coder's.
// A band that stopped at the cut of a file cut inside its scan (pad & 1, kHuffEndCut) is the file's under recode_finish's own condition,
// stated per band: it is the file's LAST segment and what the segment attempted, all bands together, has reached its byte bound -- then
// nothing behind the cut can show, the segment is complete whatever rows remain, and its bytes, clipped to the bound, may go out.  (The
// slot must be the bound's size for that: clipped to anything else the bytes are not the bound's.)  A cut end state in another segment or
// with the bound not reached, and a refusal (pad & 2, kHuffEndRefused), decline the file.  recode_finish keeps the last word at the end.
// band_counted is the same rule for a caller that keeps counts and end states only (a range read, lep_range_bands.h: `bytes` holds no
// byte of the band).
inline bool band_counted(Segment* s, const lep_huff_segment& launched, uint32_t len, const lep_huff_end& end);
inline bool band_written(Segment* s, const lep_huff_segment& launched, const uint8_t* data, uint32_t len, const lep_huff_end& end) {
    if (len > launched.out_cap) len = launched.out_cap;
    s->bytes.insert(s->bytes.end(), data, data + len);
    return band_counted(s, launched, len, end);
}
inline bool band_counted(Segment* s, const lep_huff_segment& launched, uint32_t len, const lep_huff_end& end) {
    if (len > launched.out_cap) len = launched.out_cap;
    s->written += len;
    s->coded = launched.mcu_row1;
    s->overhang = (uint32_t)end.overhang_byte | ((uint32_t)end.num_overhang_bits << 8);
    memcpy(s->last_dc, end.last_dc, sizeof s->last_dc);
    const uint32_t before = s->end.attempted;
    s->end = end;
    s->end.attempted = before + end.attempted;   // recode_finish reads the segment's count, not the band's
    if (end.pad & 2) return false;
    if (end.pad & 1) {
        if (!s->last || s->slot_cap != s->bound || s->end.attempted < s->bound) return false;
        s->coded = s->row1;
        return true;
    }
    return end.attempted <= launched.out_cap;
}

// Hand on what may go out of file f: the front segment's new bytes, and on to the next segment when the front one is complete.
// give(data, len) -> false: the receiver is gone.
template <class Give>
inline void hand_on(File* f, std::vector<Segment>& segs, Give give) {
    if (!f->writes()) return;
    for (; f->front < f->nseg; ++f->front) {
        Segment& s = segs[(size_t)(f->seg0 + f->front)];
        if (s.bytes.size() > s.given) {
            const size_t at = s.given;
            s.given = s.bytes.size();
            f->scan_byte_out = true;
            f->sunk += s.given - at;
            if (!give(s.bytes.data() + at, s.given - at)) { f->gone = true; return; }
        }
        if (!s.complete()) break;
    }
}

// Is what went out of the file (head, then `given` bytes of every segment in order) the front of the finished file `jpg`?
inline bool front_of(const File& f, const std::vector<Segment>& segs, const uint8_t* head, size_t head_len, const uint8_t* jpg, size_t jpg_len) {
    if (jpg_len < f.sunk || memcmp(jpg, head, std::min(head_len, jpg_len))) return false;
    size_t at = head_len;
    for (int q = 0; q < f.nseg; ++q) {
        const Segment& s = segs[(size_t)(f.seg0 + q)];
        const size_t k = std::min(s.given, s.bytes.size());
        if (at + k > jpg_len || (k && memcmp(jpg + at, s.bytes.data(), k))) return false;
        at += k;
    }
    return at == f.sunk;
}

}  // namespace lepbands
