// lep_batch_ranges.cc -- C ABI, layer 3: lep_decompress_batch_ranges / lep_decompress_range, part of a restored file from the thread
// segments it needs.  The header says where the head ends and where every thread segment but the last starts and ends (lep_range.h); a
// range in the head is answered from the header, and a range that touches segments gives a decode session (lep_gpu_decode_rows_*) those
// segments only -- each decodes from its own start, with its own model and no row above it, and its scan writer starts from its own
// hand-off.  The loop is lep_batch_stream.cc's: after every advance ONE scan-writer launch appends the rows each segment completed to its
// slot; then lep_gpu_pack_window_device brings down only the bytes inside each segment's window, and a segment whose written count has
// reached its window's end is retired (lep_gpu_decode_rows_retire) -- nothing in the file says at which MCU row a window ends, the bands
// find it.  The bookkeeping is lep_stream_bands.h's and lep_range_bands.h's (stepped on the CPU by tests/emu/range_bands_emu.cc); the host
// keeps counts and end states of the segments, and of their bytes only the window's, in the answer itself.
// A touched segment that ran to its end is held to the next hand-off by recode_finish's own checks; a range that reaches the tail has the
// last segment run to its end and recode_finish's tail glued behind it.  DAMAGE IN A SEGMENT THE RANGE DOES NOT TOUCH IS NOT SEEN: that
// segment is never decoded, so the range is answered where lep_decompress of the whole file fails.
// Files that are not decoded in a session, files whose extents the header does not fix, and files whose writer declined (or met a cut
// that band_counted's rule does not cover) take one lep_decompress_batch call and are cut on the host.
#include "../../include/lepton_mi355x.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "lep_batch_layout.h"
#include "lep_handles.h"
#include "lep_range.h"
#include "lep_range_bands.h"
#include "lep_stream_bands.h"
#include "lep_stream_session.h"

namespace {
using Clock = std::chrono::steady_clock;
constexpr int kSessionSegments = 16384;   // what lep_gpu_pack_window_device takes as one call

struct Ranged {   // one file whose range touches segments
    int index = 0;   // in the call's arrays
    std::unique_ptr<lep_file> f;
    lep::RecodePlan plan;
    lep_image_desc geo;
    lep_segment segs[LEP_MAX_SEGMENTS];
    lep_bytes streams[LEP_MAX_SEGMENTS];
    int nseg = 0;
    lep_range_plan rp;
    std::vector<leprange::Touched> touched;
    std::vector<uint8_t> answer;
};

struct Call {
    lep_gpu* g;
    int band;
    lep_bytes* outs;
    int32_t* status;
    lep_range_stats* stats;
    std::vector<int> whole;   // files for the whole-file path
};

size_t frame_bytes(const lep_image_desc& d) {
    size_t b = 0;
    for (int c = 0; c < d.ncomp; ++c) b += lepbatch::desc_blocks(d, c) * 128;
    return b;
}

int give(const std::vector<uint8_t>& v, lep_bytes* out) {
    out->data = (uint8_t*)malloc(v.size() ? v.size() : 1);
    if (!out->data) return LEP_OS_ERROR;
    if (!v.empty()) memcpy(out->data, v.data(), v.size());
    out->len = out->cap = v.size();
    return 0;
}

// One session: the touched segments of files[first, last) as one launch, band after band.  Non-zero: the machinery failed.
int run_session(Call& C, std::vector<Ranged>& files, size_t first, size_t last) {
    lep_gpu* g = C.g;
    const int nf = (int)(last - first);
    lep::DeviceMem mem(g);
    std::vector<lep_image_desc> dev((size_t)nf);
    std::vector<size_t> frame_off((size_t)nf);
    size_t frames_total = 0;
    for (int i = 0; i < nf; ++i) { frame_off[(size_t)i] = frames_total; frames_total += (frame_bytes(files[first + (size_t)i].geo) + 255) & ~(size_t)255; }
    void* d_frames = nullptr;
    if (int rc = mem.get(frames_total + 256, &d_frames)) return rc;
    if (int rc = lep_gpu_memset(g, d_frames, 0, frames_total)) return rc;   // (rows of segments that are not begun are never read)
    std::vector<lep_segment> dsegs;
    std::vector<uint64_t> offs(1, 0);
    std::vector<uint32_t> lens;
    std::vector<lepbands::File> bfiles((size_t)nf);
    std::vector<lepbands::Segment> bsegs;
    std::vector<leprange::Touched*> win;     // per session segment
    std::vector<const lep_bytes*> stream_of;
    std::vector<lep_huff_image> himgs((size_t)nf);
    lepbatch::OutputArena arena;
    for (int i = 0; i < nf; ++i) {
        Ranged& F = files[first + (size_t)i];
        dev[(size_t)i] = F.geo;
        lepbatch::point_components(dev[(size_t)i].blocks, F.geo.ncomp, (char*)d_frames + frame_off[(size_t)i], [&](int c) { return lepbatch::desc_blocks(F.geo, c); });
        memcpy(&himgs[(size_t)i], &F.plan.image, sizeof(lep_huff_image));
        for (int c = 0; c < 4; ++c) himgs[(size_t)i].blocks[c] = c < F.geo.ncomp ? dev[(size_t)i].blocks[c] : nullptr;
        bfiles[(size_t)i].seg0 = (int)bsegs.size(); bfiles[(size_t)i].nseg = (int)F.touched.size();
        // every segment's slot is the size it has in a whole decompress (segment 0's: what the later ones leave); only the touched get one
        uint32_t caps[LEP_MAX_SEGMENTS];
        lepbatch::RecodeSlot slots[LEP_MAX_SEGMENTS];
        lepbatch::OutputArena sizes;
        for (int q = 0; q < F.nseg; ++q) caps[q] = F.plan.segs[(size_t)q].out_cap;
        lepbatch::place_recode_segments(caps, F.nseg, &sizes, slots);
        for (leprange::Touched& t : F.touched) {
            lep_segment s = F.segs[t.q];
            s.image = i;
            dsegs.push_back(s);
            stream_of.push_back(&F.streams[t.q]);
            lens.push_back((uint32_t)F.streams[t.q].len);
            offs.push_back(offs.back() + ((F.streams[t.q].len + 255) & ~(size_t)255));
            lep_huff_segment planned;
            memcpy(&planned, &F.plan.segs[(size_t)t.q], sizeof planned);
            planned.out_cap = slots[t.q].slot;
            bsegs.emplace_back();
            lepbands::start_segment(&bsegs.back(), i, planned, arena.place(slots[t.q].slot), t.q + 1 == F.nseg, slots[t.q].bound);
            win.push_back(&t);
            C.stats->mcu_rows_begun += bsegs.back().row1 - bsegs.back().row0;
        }
        F.answer.assign((size_t)F.rp.length, 0);
        if (F.rp.head_bytes) memcpy(F.answer.data(), F.plan.head.data() + F.rp.first, (size_t)F.rp.head_bytes);
    }
    const int nseg = (int)dsegs.size();
    C.stats->segments_begun += nseg;
    void *d_streams = nullptr, *d_lens = nullptr, *d_arena = nullptr, *d_packed = nullptr, *d_answer = nullptr;
    if (int rc = mem.get((size_t)offs.back() + 256, &d_streams)) return rc;
    if (int rc = mem.get(sizeof(uint32_t) * (size_t)nseg, &d_lens)) return rc;
    {
        std::vector<uint8_t> up((size_t)offs.back());
        for (int k = 0; k < nseg; ++k) if (stream_of[(size_t)k]->len) memcpy(up.data() + offs[(size_t)k], stream_of[(size_t)k]->data, stream_of[(size_t)k]->len);
        if (!up.empty()) if (int rc = lep_gpu_memcpy_h2d(g, d_streams, up.data(), up.size())) return rc;
        if (int rc = lep_gpu_memcpy_h2d(g, d_lens, lens.data(), sizeof(uint32_t) * (size_t)nseg)) return rc;
    }
    const bool pack = lep_gpu_stream_pack(g) != 0;
    if (int rc = mem.get(arena.bytes + 256, &d_arena)) return rc;
    if (pack) if (int rc = mem.get(arena.bytes + 256, &d_packed)) return rc;
    // what a band's launches answer, in one block so that one copy fetches it: dst_off[nseg + 1] | ends[nseg] | out_len[nseg]
    const size_t o_ends = sizeof(uint64_t) * ((size_t)nseg + 1), o_len = o_ends + sizeof(lep_huff_end) * (size_t)nseg;
    const size_t answer_cap = o_len + sizeof(uint32_t) * (size_t)nseg;
    if (int rc = mem.get(answer_cap, &d_answer)) return rc;
    std::vector<uint8_t> answer(answer_cap), packed;

    lep::SessionEnd session{g};
    if (int rc = lep_gpu_decode_rows_begin(g, dev.data(), nf, dsegs.data(), nseg, (const uint8_t*)d_streams, offs.data(), (const uint32_t*)d_lens, nullptr)) return rc;
    session.open = true;
    ++C.stats->sessions;

    std::vector<lep_decode_progress> prog((size_t)nseg);
    std::vector<lep_huff_segment> launch;
    std::vector<int> which;
    std::vector<uint64_t> src_off;
    std::vector<uint32_t> skip, take;
    std::vector<int32_t> retire;
    std::vector<char> sent((size_t)nseg, 0);   // retired in the decoder
    leprange::Schedule bands(C.band);
    for (int live = nseg; live > 0;) {
        if (int rc = lep_gpu_decode_rows_advance(g, bands.height(), prog.data(), nullptr)) return rc;
        ++C.stats->advances;
        // 1. row ranges
        launch.clear(); which.clear(); src_off.clear(); skip.clear(); take.clear();
        for (int i = 0; i < nf; ++i) {
            lepbands::File& bf = bfiles[(size_t)i];
            const lep_image_desc& d = dev[(size_t)i];
            const lepbands::RowUnits units = lepbands::row_units(d, himgs[(size_t)i]);
            for (int q = 0; q < bf.nseg; ++q) {
                const int k = bf.seg0 + q;
                if (prog[(size_t)k].status > 0 && !bsegs[(size_t)k].stopped) {
                    bsegs[(size_t)k].stopped = true;
                    if (!bf.failed) { bf.failed = true; bf.fail_status = prog[(size_t)k].status; }
                }
            }
            if (!bf.writes()) continue;
            for (int q = 0; q < bf.nseg; ++q) {
                const int k = bf.seg0 + q;
                lep_huff_segment hs;
                if (win[(size_t)k]->retired) continue;
                if (!lepbands::band_segment(bsegs[(size_t)k], lepbands::complete_row(bsegs[(size_t)k], prog[(size_t)k], units.vs, d.ncomp), i, &hs)) continue;
                uint32_t sk = 0, tk = 0;
                leprange::band_window(*win[(size_t)k], bsegs[(size_t)k].written, hs.out_cap, &sk, &tk);
                launch.push_back(hs); which.push_back(k); src_off.push_back(hs.out_off); skip.push_back(sk); take.push_back(tk);
            }
        }
        // 2. one writer launch, 3. windowed pack and two copies (or a copy per window)
        const int nl = (int)launch.size();
        if (nl) {
            uint64_t* d_dst_off = (uint64_t*)d_answer;
            lep_huff_end* d_ends = (lep_huff_end*)((char*)d_answer + o_ends);
            uint32_t* d_out_len = (uint32_t*)((char*)d_answer + o_len);
            if (int rc = lep_gpu_huffman_encode_device(g, himgs.data(), nf, launch.data(), nl, (uint8_t*)d_arena, d_out_len, d_ends, nullptr)) return rc;
            ++C.stats->writer_launches;
            if (pack) if (int rc = lep_gpu_pack_window_device(g, (const uint8_t*)d_arena, src_off.data(), d_out_len, skip.data(), take.data(), nl, (uint8_t*)d_packed, arena.bytes, d_dst_off, nullptr)) return rc;
            if (int rc = lep_gpu_memcpy_d2h(g, answer.data(), d_answer, answer_cap)) return rc;
            const uint64_t* dst_off = (const uint64_t*)answer.data();
            const lep_huff_end* ends = (const lep_huff_end*)(answer.data() + o_ends);
            const uint32_t* out_len = (const uint32_t*)(answer.data() + o_len);
            if (pack) {
                if (dst_off[nl] > arena.bytes) { lep_gpu_sync(g); return LEP_GPU_ERROR; }
                packed.resize((size_t)dst_off[nl]);
                if (dst_off[nl]) if (int rc = lep_gpu_memcpy_d2h(g, packed.data(), d_packed, (size_t)dst_off[nl])) return rc;
                C.stats->scan_bytes_down += dst_off[nl];
            }
            for (int j = 0; j < nl; ++j) {
                const int k = which[(size_t)j];
                lepbands::Segment& s = bsegs[(size_t)k];
                leprange::Touched& t = *win[(size_t)k];
                Ranged& F = files[first + (size_t)s.file];
                const uint32_t len = std::min(out_len[j], launch[(size_t)j].out_cap);
                const uint32_t len_in = skip[(size_t)j] < len ? std::min(len - skip[(size_t)j], take[(size_t)j]) : 0u;   // (what window_len makes of it on the device)
                const uint64_t kept = pack ? dst_off[j + 1] - dst_off[j] : len_in;
                const uint64_t at = leprange::band_out_at(t, s.written);
                if (kept != len_in || (kept && at + kept > F.answer.size())) { lep_gpu_sync(g); return LEP_GPU_ERROR; }
                if (kept) {
                    if (pack) memcpy(F.answer.data() + at, packed.data() + dst_off[j], (size_t)kept);
                    else {
                        if (int rc = lep_gpu_memcpy_d2h(g, F.answer.data() + at, (const char*)d_arena + launch[(size_t)j].out_off + skip[(size_t)j], (size_t)kept)) return rc;
                        C.stats->scan_bytes_down += kept;
                    }
                    t.kept += kept;
                }
                if (!lepbands::band_counted(&s, launch[(size_t)j], len, ends[j])) bfiles[(size_t)s.file].declined = true;
            }
        }
        // 4. segments that need no more rows: a window that is served, a writer that ended at a cut, a file that failed or was declined
        retire.clear();
        live = 0;
        for (int k = 0; k < nseg; ++k) {
            lepbands::Segment& s = bsegs[(size_t)k];
            leprange::Touched& t = *win[(size_t)k];
            const lepbands::File& bf = bfiles[(size_t)s.file];
            const bool runs = prog[(size_t)k].status == -1 && !sent[(size_t)k];
            const bool served = !s.complete() && leprange::window_reached(t, s.written);
            if (!t.settled && (!runs || served || s.complete() || !bf.writes())) {
                const lepbands::RowUnits units = lepbands::row_units(dev[(size_t)s.file], himgs[(size_t)s.file]);
                t.settled = true;
                C.stats->mcu_rows_decoded += lepbands::complete_row(s, prog[(size_t)k], units.vs, dev[(size_t)s.file].ncomp) - s.row0;
                if (served && bf.writes()) { t.retired = true; ++C.stats->segments_retired; }
            }
            if (runs && t.settled) { retire.push_back(k); sent[(size_t)k] = 1; }
            else if (runs) ++live;
        }
        if (!retire.empty()) if (int rc = lep_gpu_decode_rows_retire(g, retire.data(), (int)retire.size())) return rc;
    }
    session.open = false;
    if (int rc = lep_gpu_decode_rows_end(g)) return rc;
    for (int i = 0; i < nf; ++i) {
        Ranged& F = files[first + (size_t)i];
        lepbands::File& bf = bfiles[(size_t)i];
        int rc = 0;
        if (bf.failed) rc = bf.fail_status;
        else if (bf.declined) rc = LEP_GPU_PATH_DECLINED;
        else
            rc = leprange::finish(
                F.rp, F.touched, &bsegs[(size_t)bf.seg0],
                [&](int q, const lep_huff_end& end, uint64_t bytes, bool last_of_file) {
                    if (int r = lep::recode_segment_end_declined(F.plan, (size_t)q, last_of_file, end)) return r;
                    return lep::recode_segment_end_check(F.f->lf, F.plan, (size_t)q, &end, bytes);
                },
                [&](uint64_t bytes_in_front, std::vector<uint8_t>* tail, uint64_t* at) {
                    *at = std::min<uint64_t>(bytes_in_front, F.plan.scan_bound);
                    lep::recode_tail(&F.f->lf, F.plan, *at, tail);
                },
                &F.answer);
        if (rc == LEP_GPU_PATH_DECLINED) {   // correct, not economical: the whole file, cut on the host
            C.whole.push_back(F.index);
            --C.stats->files_ranged; ++C.stats->files_whole;
        } else {
            C.status[F.index] = rc ? rc : give(F.answer, &C.outs[F.index]);
        }
        F.answer = std::vector<uint8_t>();
        F.f.reset();
    }
    return 0;
}
}  // namespace

extern "C" int lep_decompress_batch_ranges(lep_gpu* g, const lep_bytes* leps, const lep_range* ranges, int n, int band_mcu_rows, lep_bytes* outs, int32_t* status,
                                           const lep_batch_options* opt, lep_range_stats* stats) {
    if (!g) return LEP_GPU_ERROR;
    if (!outs || !status || n < 0 || (n && (!leps || !ranges))) return LEP_ASSERTION_FAILURE;
    lep_range_stats local;
    if (!stats) stats = &local;
    memset(stats, 0, sizeof *stats);
    const Clock::time_point t0 = Clock::now();
    Call C{g, band_mcu_rows, outs, status, stats, {}};
    int session_files = 64;
    if (const char* e = getenv("LEP_STREAM_SESSION_FILES")) if (atoi(e) > 0) session_files = atoi(e);
    std::vector<Ranged> files;
    for (int i = 0; i < n; ++i) {
        status[i] = LEP_CODING_ERROR;
        outs[i] = lep_bytes{nullptr, 0, 0};
        lep_file* f = nullptr;
        Ranged F;
        if (lep_file_open(leps[i].data, leps[i].len, &f) == 0) {
            F.f.reset(f);
            if (lep::streams_in_session(f, leps[i].data, leps[i].len, &F.plan, F.segs, F.streams, &F.nseg) &&
                lep_file_describe_into(f, nullptr, (size_t)-1, &F.geo) == 0) {
                lep::RangeParts parts;
                const lep::RangeAnswer a = lep::range_plan(&f->lf, F.plan, ranges[i].first, ranges[i].length, &parts);
                lep::fill_range_plan(parts, a, true, &F.rp);
                if (parts.nseg > 0 && a.first_seg < 0) {   // in the head, or empty: no segment, no launch
                    std::vector<uint8_t> part;
                    if (a.head_bytes) part.assign(F.plan.head.begin() + (ptrdiff_t)a.first, F.plan.head.begin() + (ptrdiff_t)(a.first + a.head_bytes));
                    status[i] = give(part, &outs[i]);
                    ++stats->files_no_decode;
                    continue;
                }
                if (parts.nseg > 0 && parts.sizes_known) {
                    leprange::touched_of(F.rp, &F.touched);
                    F.index = i;
                    stats->segments_total += F.nseg;
                    files.push_back(std::move(F));
                    continue;
                }
            }
        }
        C.whole.push_back(i);   // (a file that does not parse gets its exit code from lep_decompress_batch)
    }
    stats->files_ranged = (int)files.size();
    stats->files_whole = (int)C.whole.size();
    int rc = 0;
    for (size_t first = 0; first < files.size() && !rc;) {
        size_t last = first;
        int segs = 0;
        while (last < files.size() && (int)(last - first) < session_files && segs + (int)files[last].touched.size() <= kSessionSegments) segs += (int)files[last++].touched.size();
        rc = run_session(C, files, first, last);
        first = last;
    }
    files.clear();
    if (!rc && !C.whole.empty()) {
        std::sort(C.whole.begin(), C.whole.end());
        const std::vector<int>& whole = C.whole;
        std::vector<lep_bytes> in(whole.size()), full(whole.size(), lep_bytes{nullptr, 0, 0});
        std::vector<int32_t> st(whole.size(), LEP_CODING_ERROR);
        for (size_t k = 0; k < whole.size(); ++k) in[k] = leps[whole[k]];
        rc = lep_decompress_batch(g, in.data(), (int)whole.size(), full.data(), st.data(), opt, nullptr);
        for (size_t k = 0; k < whole.size(); ++k) {
            const int i = whole[k];
            status[i] = rc ? rc : st[k];
            if (!rc && st[k] == 0 && full[k].data) {
                const uint64_t size = full[k].len, lo = std::min<uint64_t>(ranges[i].first, size);
                const uint64_t room = size - lo, len = (ranges[i].length == 0 || ranges[i].length > room) ? room : ranges[i].length;
                status[i] = give(std::vector<uint8_t>(full[k].data + lo, full[k].data + lo + len), &outs[i]);
            }
            if (full[k].data) lep_free(full[k].data);
        }
    }
    stats->wall_s = std::chrono::duration<double>(Clock::now() - t0).count();
    return rc;
}

extern "C" int lep_decompress_range(lep_gpu* g, const uint8_t* lepdata, size_t len, uint64_t first, uint64_t length, lep_bytes* out) {
    if (!out) return LEP_ASSERTION_FAILURE;
    const lep_bytes in = {const_cast<uint8_t*>(lepdata), len, len};
    const lep_range r = {first, length};
    int32_t status = LEP_CODING_ERROR;
    if (int rc = lep_decompress_batch_ranges(g, &in, &r, 1, 0, out, &status, nullptr, nullptr)) return rc;
    return status;
}
