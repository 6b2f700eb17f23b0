// lep_range.h -- host only, no device: where a byte range of the restored file lies.  A file the split re-coder plans is its head
// (RecodePlan::head), one extent per thread segment, and the tail (misplaced restart markers, the rest of the header, the garbage).
// Every segment but the last writes exactly segment_size bytes -- recode_finish holds it to that (recode_segment_end_check) --, so the
// extents in front of the last segment's start are known from the header.  The last segment's end is not: seg_len of the last segment
// is "to the tail" under the assumption that the file has jpeg_size bytes and no bound cuts its tail, and is flagged as such.  A
// caller finds the true end by running the segment to its end.  A window that reaches into the last segment is therefore open to where
// the garbage starts (scan_bound): its take may run past the segment's bytes, and what it then misses is the tail's (recode_tail).  A
// range that starts behind the last segment's bytes still touches that segment -- with a window that takes nothing.
// A -startbyte / -trunc file ('Y') counts in its own bytes: its head is the prefix garbage, jpeg_size its length.
#pragma once
#include <stdint.h>

#include <algorithm>

#include <string.h>

#include "../../include/lepton_mi355x.h"
#include "lep_container.h"

namespace lep {

constexpr int kRangeSegments = 16;

struct RangeParts {
    uint64_t jpeg_size = 0, head_len = 0;
    int nseg = 0;                              // 0: not a planned file (no extents)
    uint64_t seg_first[kRangeSegments] = {0};  // first byte of segment q in the restored file
    uint64_t seg_len[kRangeSegments] = {0};    // its byte count; the last segment's: to the tail
    bool sizes_known = false;                  // every extent in front of the last segment is one the header fixes
    bool last_len_known = false;               // never proved from the header: false
    uint64_t tail_len = 0;                     // recode_tail_bytes
    uint64_t scan_bound = 0;                   // bytes the file may hold in front of the trailing garbage (RecodePlan::scan_bound)
};

struct RangeAnswer {
    uint64_t first = 0, length = 0;            // the range, clipped to the file
    uint64_t head_bytes = 0;                   // bytes of the head it holds
    int first_seg = -1, last_seg = -1;         // segments it touches (-1: none)
    uint64_t skip[kRangeSegments] = {0}, take[kRangeSegments] = {0};   // per touched segment, from the segment's first byte
    bool reaches_last = false;                 // it reaches behind the last segment's start: that segment is needed (to its end, if the window outlasts it)
};

inline RangeParts range_parts(const LepFile& lf, const RecodePlan& plan) {
    RangeParts p;
    p.jpeg_size = lf.jpeg_size;
    if (!plan.gpu_ok || plan.segs.empty() || plan.segs.size() > (size_t)kRangeSegments || plan.segs.size() != lf.segs.size()) return p;
    p.head_len = plan.head.size();
    p.nseg = (int)plan.segs.size();
    p.tail_len = recode_tail_bytes(lf, plan);
    p.scan_bound = plan.scan_bound;
    p.sizes_known = true;
    uint64_t at = p.head_len;
    for (int q = 0; q < p.nseg; ++q) {
        p.seg_first[q] = at;
        if (q + 1 < p.nseg) {
            p.seg_len[q] = lf.segs[(size_t)q].segment_size;
            if (!recode_segment_size_known(lf, plan, (size_t)q)) p.sizes_known = false;
        } else {
            p.seg_len[q] = p.jpeg_size > at + p.tail_len ? p.jpeg_size - at - p.tail_len : 0;
        }
        at += p.seg_len[q];
    }
    if (p.seg_first[p.nseg - 1] > p.jpeg_size) p.sizes_known = false;   // (hand-offs that claim more than the file holds)
    return p;
}

// length == 0: to the end.  The range is clipped to jpeg_size; first >= jpeg_size is the empty answer.
inline RangeAnswer range_of(const RangeParts& p, uint64_t first, uint64_t length) {
    RangeAnswer a;
    if (first >= p.jpeg_size) { a.first = p.jpeg_size; return a; }
    const uint64_t room = p.jpeg_size - first;
    a.first = first;
    a.length = (length == 0 || length > room) ? room : length;
    const uint64_t end = a.first + a.length;
    if (a.first < p.head_len) a.head_bytes = std::min(end, p.head_len) - a.first;
    for (int q = 0; q < p.nseg; ++q) {
        // The last segment's window is open to where the garbage starts, and the segment is touched by whatever reaches behind its first
        // byte: a range that lies in the tail needs the segment's true end (its window then takes nothing).
        const bool last = q + 1 == p.nseg;
        const uint64_t s0 = p.seg_first[q], s1 = last ? std::max(s0, std::min(p.jpeg_size, p.scan_bound)) : s0 + p.seg_len[q];
        const uint64_t lo = std::max(a.first, s0), hi = std::min(end, s1);
        if (last ? end <= s0 : hi <= lo) continue;
        if (a.first_seg < 0) a.first_seg = q;
        a.last_seg = q;
        a.skip[q] = std::min(lo, s1) - s0;
        a.take[q] = hi > lo ? hi - lo : 0;
        if (last) a.reaches_last = true;
    }
    return a;
}

inline RangeAnswer range_plan(LepFile* lf, const RecodePlan& plan, uint64_t first, uint64_t length, RangeParts* parts = nullptr) {
    const RangeParts p = range_parts(*lf, plan);
    if (parts) *parts = p;
    return range_of(p, first, length);
}


inline void fill_range_plan(const RangeParts& p, const RangeAnswer& a, bool in_session, lep_range_plan* out) {
    memset(out, 0, sizeof *out);
    out->in_session = in_session ? 1 : 0;
    out->nseg = p.nseg;
    out->jpeg_size = p.jpeg_size; out->head_len = p.head_len;
    out->sizes_known = p.sizes_known ? 1 : 0; out->last_len_known = p.last_len_known ? 1 : 0;
    out->tail_len = p.tail_len; out->scan_bound = p.scan_bound;
    out->first = a.first; out->length = a.length; out->head_bytes = a.head_bytes;
    out->first_seg = a.first_seg; out->last_seg = a.last_seg;
    out->reaches_last = a.reaches_last ? 1 : 0;
    for (int q = 0; q < kRangeSegments; ++q) {
        out->seg_first[q] = p.seg_first[q]; out->seg_len[q] = p.seg_len[q];
        out->win_skip[q] = a.skip[q]; out->win_take[q] = a.take[q];
    }
}

}  // namespace lep
