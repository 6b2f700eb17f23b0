// lep_stream.cc -- C ABI, layer 3: lep_decompress_stream, a whole file decoded in a session of the resumable decoder
// (lep_gpu_decode_rows_*, lep_gpu.hip) and re-coded on the host as its rows arrive.  A file of its own because, unlike lep_api.cc, it
// needs the GPU runtime's device-memory and session calls: lep_api.cc stays linkable with the two host-variant coder calls alone.
#include "../../include/lepton_mi355x.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "lep_handles.h"
#include "lep_range.h"
#include "lep_stream_bands.h"
#include "lep_stream_session.h"

extern "C" {

// Is this .lep one that lep_decompress_stream / lep_decompress_batch_stream decode in a session (1) or hand to lep_decompress whole (0)?
// Host only.  A file that does not parse answers its exit code -- bar LEP_ASSERTION_FAILURE, which is 1: such a file is not streamed, 0.
int lep_file_streams_in_session(const uint8_t* lepdata, size_t len) {
    lep_file* f = nullptr;
    if (int rc = lep_file_open(lepdata, len, &f)) return rc == LEP_ASSERTION_FAILURE ? 0 : rc;
    std::unique_ptr<lep_file> hold(f);
    lep::RecodePlan plan;
    lep_segment segs[LEP_MAX_SEGMENTS];
    lep_bytes streams[LEP_MAX_SEGMENTS];
    int n = 0;
    return lep::streams_in_session(f, lepdata, len, &plan, segs, streams, &n) ? 1 : 0;
}

// Where a byte range of the restored file lies (lep_range.h).  Host only.  A file that is not decoded in a session has no extents.
int lep_file_range_plan(const uint8_t* lepdata, size_t len, uint64_t first, uint64_t length, lep_range_plan* out) {
    if (!out) return LEP_ASSERTION_FAILURE;
    memset(out, 0, sizeof *out);
    out->first_seg = out->last_seg = -1;
    lep_file* f = nullptr;
    if (int rc = lep_file_open(lepdata, len, &f)) return rc;
    std::unique_ptr<lep_file> hold(f);
    lep::RecodePlan plan;
    lep_segment segs[LEP_MAX_SEGMENTS];
    lep_bytes streams[LEP_MAX_SEGMENTS];
    int n = 0;
    const bool in_session = lep::streams_in_session(f, lepdata, len, &plan, segs, streams, &n);
    if (!in_session) plan.gpu_ok = false;
    lep::RangeParts parts;
    const lep::RangeAnswer a = lep::range_plan(&f->lf, plan, first, length, &parts);
    lep::fill_range_plan(parts, a, in_session, out);
    return 0;
}

// lep_decompress with the bytes handed on as they become final (include/lepton_mi355x.h).  The decode is a session
// (lep_gpu_decode_rows_*): after every advance the block rows the segments completed are fetched into the host frame and the MCU rows
// they complete are coded by a SegmentRowCoder per segment; recode_finish, over the same bytes, supplies the checks and the tail.
// Streamed: every single file the split re-coder plans (lep::streams_in_session) -- whole files and -startbyte / -trunc slices, one to
// three components, cut inside the scan or not.  A cut file's coders read what the re-coder reads behind the cut (RowCoder::mcu_row) and
// are bound by the segments' byte bounds, so nothing goes out that the finished file does not start with; the front check below stays.
using lep::DeviceMem;
using lep::SessionEnd;

static int decompress_whole_to_sink(lep_gpu* g, const uint8_t* lepdata, size_t len, lep_sink sink, void* user) {
    lep_bytes out = {nullptr, 0, 0};
    if (int rc = lep_decompress(g, lepdata, len, &out)) return rc;
    const int stop = sink(user, out.data, out.len);
    lep_free(out.data);
    return stop ? LEP_OS_ERROR : 0;
}

int lep_decompress_stream(lep_gpu* g, const uint8_t* lepdata, size_t len, int band_mcu_rows, lep_sink sink, void* user, lep_stream_stats* stats) {
    if (!g) return LEP_GPU_ERROR;
    if (!sink) return LEP_ASSERTION_FAILURE;
    lep_stream_stats local;
    if (!stats) stats = &local;
    memset(stats, 0, sizeof *stats);
    lep_file* f = nullptr;
    if (int rc = lep_file_open(lepdata, len, &f)) return rc;
    std::unique_ptr<lep_file> hold(f);
    lep::LepFile& lf = f->lf;
    lep::JpegFile& jf = lf.jpeg;
    lep::RecodePlan plan;
    lep_image_desc d;
    lep_segment segs[LEP_MAX_SEGMENTS];
    lep_bytes streams[LEP_MAX_SEGMENTS];
    int n = 0;
    if (!lep::streams_in_session(f, lepdata, len, &plan, segs, streams, &n)) {
        hold.reset();
        return decompress_whole_to_sink(g, lepdata, len, sink, user);
    }
    lep_file_describe(f, &d);

    // device side: a zeroed frame, the streams back to back, their lengths
    DeviceMem mem(g);
    lep_image_desc dev = d;
    size_t plane_bytes[LEP_MAX_COMPONENTS] = {0, 0, 0};
    for (int c = 0; c < d.ncomp; ++c) {
        plane_bytes[c] = (size_t)d.width_blocks[c] * d.height_blocks[c] * 128;
        void* p = nullptr;
        if (int rc = mem.get(plane_bytes[c] + 256, &p)) return rc;
        if (int rc = lep_gpu_memset(g, p, 0, plane_bytes[c])) return rc;
        dev.blocks[c] = (int16_t*)p;
    }
    uint64_t offs[LEP_MAX_SEGMENTS + 1] = {0};
    uint32_t lens[LEP_MAX_SEGMENTS];
    for (int s = 0; s < n; ++s) { lens[s] = (uint32_t)streams[s].len; offs[s + 1] = offs[s] + ((streams[s].len + 255) & ~(size_t)255); }
    void *d_streams = nullptr, *d_lens = nullptr;
    if (int rc = mem.get((size_t)offs[n] + 256, &d_streams)) return rc;
    if (int rc = mem.get(sizeof lens, &d_lens)) return rc;
    for (int s = 0; s < n; ++s)
        if (streams[s].len) if (int rc = lep_gpu_memcpy_h2d(g, (uint8_t*)d_streams + offs[s], streams[s].data, streams[s].len)) return rc;
    if (int rc = lep_gpu_memcpy_h2d(g, d_lens, lens, sizeof(uint32_t) * (size_t)n)) return rc;

    SessionEnd session{g};
    if (int rc = lep_gpu_decode_rows_begin(g, &dev, 1, segs, n, (const uint8_t*)d_streams, offs, (const uint32_t*)d_lens, nullptr)) return rc;
    session.open = true;

    uint64_t sunk = 0;
    auto give = [&](const uint8_t* p, size_t k) -> bool {
        if (!k) return true;
        sunk += k;
        return sink(user, p, k) == 0;
    };
    if (!give(plan.head.data(), plan.head.size())) return LEP_OS_ERROR;
    std::vector<std::unique_ptr<lep::SegmentRowCoder>> coders;
    for (int s = 0; s < n; ++s) coders.emplace_back(new lep::SegmentRowCoder(&lf, plan, (size_t)s));
    std::vector<size_t> given((size_t)n, 0);      // bytes of segment s the sink has
    int front = 0;                                // first segment whose bytes are not all out
    int fetched[LEP_MAX_SEGMENTS][LEP_MAX_COMPONENTS] = {{0}};   // rows_done as of the last fetch
    lep_decode_progress prog[LEP_MAX_SEGMENTS];
    int vs[LEP_MAX_COMPONENTS];
    lepbands::block_rows_per_mcu_row(d, vs);                                   // where a segment's rows start in every component (the fetch)
    const lepbands::RowUnits units = lepbands::row_units(d, plan.image);      // the plan's rows, which the coders count in
    bool failed = false, scan_byte_out = false;
    for (int running = 1; running > 0;) {
        stats->bytes_before_last_advance = sunk;
        if (int rc = lep_gpu_decode_rows_advance(g, failed ? 0 : band_mcu_rows, prog, &running)) return rc;
        ++stats->advances;
        if (!scan_byte_out) stats->advances_before_first_scan_byte = stats->advances;
        for (int s = 0; s < n; ++s) if (prog[s].status > 0) failed = true;
        if (failed) continue;   // (nothing more goes out; the launch is run to its end for the exit code lep_decompress gives)
        for (int s = 0; s < n; ++s) {
            int complete = coders[(size_t)s]->end_row();
            for (int c = 0; c < d.ncomp; ++c) {
                const int r0 = fetched[s][c] ? fetched[s][c] : std::min(segs[s].luma_y_start / vs[0] * vs[c], prog[s].rows_done[c]), r1 = prog[s].rows_done[c];
                if (r1 > r0) {
                    const size_t row_bytes = (size_t)d.width_blocks[c] * 128;
                    if (int rc = lep_gpu_memcpy_d2h(g, (char*)d.blocks[c] + (size_t)r0 * row_bytes, (const char*)dev.blocks[c] + (size_t)r0 * row_bytes, (size_t)(r1 - r0) * row_bytes)) return rc;
                    fetched[s][c] = r1;
                }
                if (prog[s].status != 0) complete = std::min(complete, prog[s].rows_done[c] / units.vs[c]);
            }
            coders[(size_t)s]->code_rows(complete);
        }
        for (; front < n; ++front) {
            const std::vector<uint8_t>& b = coders[(size_t)front]->bytes();
            if (b.size() > given[(size_t)front]) {
                scan_byte_out = true;
                const size_t at = given[(size_t)front];
                given[(size_t)front] = b.size();
                if (!give(b.data() + at, b.size() - at)) return LEP_OS_ERROR;
            }
            if (coders[(size_t)front]->next_row() < coders[(size_t)front]->end_row()) break;
        }
    }
    session.open = false;
    if (int rc = lep_gpu_decode_rows_end(g)) return rc;
    if (failed) {
        for (int s = 0; s < n; ++s) if (prog[s].status > 0) return prog[s].status;
        return LEP_ASSERTION_FAILURE;
    }
    // the file as lep_decompress builds it: recode_finish over these segments' bytes (its checks of the end states included), the
    // one-thread re-coder where that declines
    std::vector<uint8_t> jpg;
    {
        std::vector<lep_huff_end> ends((size_t)n);
        std::vector<std::pair<const uint8_t*, size_t>> sb;
        for (int s = 0; s < n; ++s) { coders[(size_t)s]->end_state(&ends[(size_t)s]); sb.emplace_back(coders[(size_t)s]->bytes().data(), coders[(size_t)s]->bytes().size()); }
        if (n < 2 || lep::recode_finish(&lf, plan, sb, ends.data(), &jpg) != 0) {
            jpg.clear();
            if (int rc = lep::recode_jpeg(&lf, &jpg)) return rc;
        }
    }
    // what went out must be the front of it (a file the split form codes differently from the one-thread walk: none is known)
    size_t at = 0;
    if (jpg.size() < sunk || memcmp(jpg.data(), plan.head.data(), std::min(plan.head.size(), jpg.size()))) return LEP_ASSERTION_FAILURE;
    at = plan.head.size();
    for (int s = 0; s < n; ++s) {
        const std::vector<uint8_t>& b = coders[(size_t)s]->bytes();
        const size_t k = std::min(given[(size_t)s], b.size());
        if (at + k > jpg.size() || (k && memcmp(jpg.data() + at, b.data(), k))) return LEP_ASSERTION_FAILURE;
        at += k;
    }
    if (at != sunk) return LEP_ASSERTION_FAILURE;
    if (!give(jpg.data() + at, jpg.size() - at)) return LEP_OS_ERROR;
    return 0;
}

}  // extern "C"

bool lep::streams_in_session(lep_file* f, const uint8_t* lepdata, size_t len, RecodePlan* plan, lep_segment* segs, lep_bytes* streams, int* nseg) {
    LepFile& lf = f->lf;
    *nseg = 0;
    // Every single file the split re-coder plans: 'Z' and 'Y' (a -startbyte / -trunc slice), one to three components, cut inside the scan
    // or not, with or without restart intervals.  What recode_prepare does not plan or declines stays out by itself: progressive files,
    // sequential frames in several scans, cut files with restart intervals or one component, the layouts it sends to the host re-coder.
    const bool chained = lep_chained_file_follows(lepdata, len, lep_file_consumed(f)) != 0;
    if (chained || recode_prepare(&lf, plan) != 0 || !plan->gpu_ok) return false;
    const int n = lep_file_segments(f, segs, streams, 0);
    if (n <= 0 || (size_t)n != plan->segs.size()) return false;
    *nseg = n;
    return true;
}
