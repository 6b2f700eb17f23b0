// lep_range_bands.h -- host only: the bookkeeping of a range read (lep_decompress_batch_ranges, lep_batch_ranges.cc; stepped on the CPU by
// tests/emu/range_bands_emu.cc) beside lep_stream_bands.h's.  A ranged file gives the session only the thread segments its range touches
// (lep_range_plan); each of them has a window, counted from the segment's first byte.  Band after band the writer appends to the
// segment's slot as in a streamed decompress; of a band's bytes only those inside the window are kept (band_window: what the windowed
// pack is told), they go straight to their place in the answer (band_out_at), and a segment whose written count has reached its
// window's end is retired (window_reached).  lepbands::Segment::bytes stays empty: counts and end states only (lepbands::band_counted).
// At the end (finish) every touched segment that ran to its end is held to the next hand-off, and a range that reaches the tail has it
// glued behind the last segment's true end.  Nothing here touches a device.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/lepton_mi355x.h"
#include "lep_stream_bands.h"

namespace leprange {

// band heights of a call: a fixed height, or the library's schedule 1, 2, 4, ... MCU rows -- after k advances 2^k - 1 rows: at most
// ceil(log2 rows) + 1 advances for `rows` rows, and fewer than twice the rows that were needed
struct Schedule {
    int fixed = 0, next = 1;
    explicit Schedule(int band_mcu_rows) : fixed(band_mcu_rows > 0 ? band_mcu_rows : 0) {}
    int height() {
        if (fixed) return fixed;
        const int h = next;
        if (next < (1 << 28)) next *= 2;
        return h;
    }
};

struct Touched {                 // one touched segment of a ranged file, beside its lepbands::Segment
    int q = 0;                   // the segment in its file
    uint64_t skip = 0, take = 0; // its window, from the segment's first byte
    uint64_t out_at = 0;         // where the window's first byte stands in the file's answer
    bool retired = false;
    bool settled = false;        // finished or retired, and its rows counted
    uint64_t kept = 0;           // bytes of the window that were kept
    uint64_t end() const { return skip + take; }
};

// The touched segments of a planned range, in file order.
inline void touched_of(const lep_range_plan& rp, std::vector<Touched>* out) {
    for (int q = rp.first_seg; q >= 0 && q <= rp.last_seg; ++q) {
        if (!rp.win_take[q] && q + 1 != rp.nseg) continue;   // (the last segment is needed for its true end even where its window takes nothing)
        Touched t;
        t.q = q; t.skip = rp.win_skip[q]; t.take = rp.win_take[q];
        t.out_at = t.take ? rp.seg_first[q] + t.skip - rp.first : 0;
        out->push_back(t);
    }
}

// A band's bytes are the segment's bytes [written, written + len), len <= cap: which of them lie in the window.  take 0: none.
inline void band_window(const Touched& t, uint64_t written, uint32_t cap, uint32_t* skip, uint32_t* take) {
    const uint64_t lo = std::max(t.skip, written), hi = std::min(t.end(), written + cap);
    *skip = hi > lo ? (uint32_t)(lo - written) : 0u;
    *take = hi > lo ? (uint32_t)(hi - lo) : 0u;
}
// ... and where the first of them stands in the answer
inline uint64_t band_out_at(const Touched& t, uint64_t written) { return t.out_at + (std::max(t.skip, written) - t.skip); }
// written: the segment's count after a band.  true: the window is served, the segment needs no more rows
inline bool window_reached(const Touched& t, uint64_t written) { return written >= t.end(); }

// The end of one ranged file whose touched segments are all finished or retired.  `answer` holds rp.length bytes with the head's and the
// windows' bytes in place.  check(q, end, bytes, last_of_file) -> 0, LEP_GPU_PATH_DECLINED or LEP_ASSERTION_FAILURE: recode_finish's
// checks for a segment that ran to its end; tail(bytes_in_front, &bytes, &first): what recode_finish writes behind the last segment and
// where it starts.  The tail is asked for when the last segment is touched and either ran to its end or was retired with the range
// reaching past its window (a window ends at scan_bound: behind that stands the garbage, whatever the segment wrote).
// 0: the answer is final (shorter than rp.length where the file is).  LEP_GPU_PATH_DECLINED: the whole-file path decides.
template <class Check, class Tail>
inline int finish(const lep_range_plan& rp, const std::vector<Touched>& touched, const lepbands::Segment* segs, Check check, Tail tail, std::vector<uint8_t>* answer) {
    for (size_t i = 0; i < touched.size(); ++i) {
        const Touched& t = touched[i];
        const lepbands::Segment& s = segs[i];
        if (t.retired) continue;
        if (!s.complete()) return LEP_ASSERTION_FAILURE;
        if (int rc = check(t.q, s.end, (uint64_t)s.written, t.q + 1 == rp.nseg)) return rc;
    }
    if (touched.empty() || touched.back().q + 1 != rp.nseg) return 0;
    const Touched& t = touched.back();
    const lepbands::Segment& s = segs[touched.size() - 1];
    const uint64_t range_end = rp.first + rp.length;
    if (t.retired && range_end <= rp.seg_first[t.q] + t.end()) return 0;
    std::vector<uint8_t> tb;
    uint64_t t0 = 0;
    tail(rp.seg_first[t.q] + s.written, &tb, &t0);
    const uint64_t size = t0 + tb.size();
    const uint64_t lo = std::max(t0, rp.first), hi = std::min(size, range_end);
    if (hi > lo) memcpy(answer->data() + (lo - rp.first), tb.data() + (lo - t0), (size_t)(hi - lo));
    if (size < range_end) answer->resize(size > rp.first ? (size_t)(size - rp.first) : 0);
    return 0;
}

}  // namespace leprange
