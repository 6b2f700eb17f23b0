// lep_batch_stream.cc -- C ABI, layer 3: lep_decompress_batch_stream, the layer between a decode session and a socket.  Many files are
// decoded in one session of the resumable decoder (lep_gpu_decode_rows_*); after every advance the MCU rows that every thread segment
// completed are written by the lane scan writer on the device (lep_gpu_huffman_encode_device: one launch per band, every segment from the
// end state of its band before), the band's new bytes are moved back to back (lep_gpu_pack_device) and come down in two copies; only scan
// bytes cross PCIe.  The band bookkeeping is lep_stream_bands.h's (stepped on the CPU by tests/emu/stream_bands_emu.cc and stream_layouts_emu.cc); here are the
// device memory, the launches and the copies.  Streamed: every single file the split re-coder plans (lep::streams_in_session) -- whole files
// and -startbyte / -trunc slices, one to three components, cut inside the scan or not.  Files that are not streamed take one
// lep_decompress_batch call.
// A file cut inside its scan needs nothing done to its frame in front of a band's writer launch, as it needs nothing in front of
// lep_decompress_batch's one scan launch (launch_decompress_chunk clears behind the cut for PROGRESSIVE files of one segment only, and
// those are not streamed): the session's frames start zero-filled, the decoder stores nothing behind the cut, and the lane writer
// itself stops at the first block at or behind trunc_bc (a row's first block apart, the reference's decode_row rule: lep_huff_simt.h
// code_mcus) and says so in its end state -- which band_written (lep_stream_bands.h) weighs band by band.
#include "../../include/lepton_mi355x.h"

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "lep_batch_layout.h"
#include "lep_handles.h"
#include "lep_stream_bands.h"
#include "lep_stream_session.h"

namespace {
using Clock = std::chrono::steady_clock;
constexpr int kSessionSegments = 16384;   // what lep_gpu_pack_device takes as one call

struct Streamed {   // one file that is decoded in a session
    int index = 0;  // in the call's arrays
    std::unique_ptr<lep_file> f;
    lep::RecodePlan plan;
    lep_image_desc geo;
    lep_segment segs[LEP_MAX_SEGMENTS];
    lep_bytes streams[LEP_MAX_SEGMENTS];
    int nseg = 0;
    int first_scan_advance = 0;   // the advance behind which its first scan byte went out (0: none yet)
    int front_last_advance = 0;   // the last advance its front segment (segment 0) took part in
};

struct Call {
    lep_gpu* g;
    int band;
    lep_batch_sink sink;
    void* user;
    int32_t* status;
    lep_batch_stream_stats* stats;
    Clock::time_point t0;
    bool first_piece = false;
    void piece_with_scan_bytes() {
        if (first_piece) return;
        first_piece = true;
        stats->first_piece_s = std::chrono::duration<double>(Clock::now() - t0).count();
    }
};

size_t frame_bytes(const lep_image_desc& d) {
    size_t b = 0;
    for (int c = 0; c < d.ncomp; ++c) b += lepbatch::desc_blocks(d, c) * 128;
    return b;
}

// The end of one streamed file: recode_finish over the segments' bytes and end states -- the hand-off checks and the tail -- or, where the
// writer declined or the finish did not succeed, the frame fetched and the host re-coder; what went out must be the front of either.
int finish_file(Call& C, Streamed& F, lepbands::File& bf, std::vector<lepbands::Segment>& segs, const char* d_frame) {
    if (bf.failed) return bf.fail_status;
    if (bf.gone) return LEP_OS_ERROR;
    lep::LepFile& lf = F.f->lf;
    std::vector<uint8_t> jpg;
    bool host = bf.declined;
    if (!host) {
        std::vector<lep_huff_end> ends((size_t)F.nseg);
        std::vector<std::pair<const uint8_t*, size_t>> sb;
        for (int q = 0; q < F.nseg; ++q) {
            const lepbands::Segment& s = segs[(size_t)(bf.seg0 + q)];
            ends[(size_t)q] = s.end;
            sb.emplace_back(s.bytes.data(), s.bytes.size());
        }
        // (declined, or a hand-off check that failed: the one-thread re-coder decides, as it does for lep_decompress)
        if (lep::recode_finish(&lf, F.plan, sb, ends.data(), &jpg) != 0) host = true;
    }
    if (host) {   // the one case in which a frame crosses PCIe
        lep_image_desc d;
        if (int rc = lep_file_describe(F.f.get(), &d)) return rc;
        size_t off = 0;
        for (int c = 0; c < d.ncomp; ++c) {
            const size_t bytes = lepbatch::desc_blocks(d, c) * 128;
            if (int rc = lep_gpu_memcpy_d2h(C.g, d.blocks[c], d_frame + off, bytes)) return rc;
            off += bytes;
        }
        C.stats->frame_bytes_down += off;
        jpg.clear();
        if (int rc = lep::recode_jpeg(&lf, &jpg)) return rc;
    }
    if (!lepbands::front_of(bf, segs, F.plan.head.data(), F.plan.head.size(), jpg.data(), jpg.size())) return LEP_ASSERTION_FAILURE;
    if (jpg.size() > bf.sunk) {
        C.piece_with_scan_bytes();
        if (C.sink(C.user, F.index, jpg.data() + bf.sunk, jpg.size() - (size_t)bf.sunk)) return LEP_OS_ERROR;
    }
    return 0;
}

// One session: files[first, last) decoded as one launch, band after band.  Non-zero: the machinery failed (the files keep the status they have).
int run_session(Call& C, std::vector<Streamed>& files, size_t first, size_t last) {
    lep_gpu* g = C.g;
    const int nf = (int)(last - first);
    lep::DeviceMem mem(g);
    // frames (zero-filled) and streams: device memory of the call
    std::vector<lep_image_desc> dev((size_t)nf);
    std::vector<size_t> frame_off((size_t)nf);
    size_t frames_total = 0;
    for (int i = 0; i < nf; ++i) { frame_off[(size_t)i] = frames_total; frames_total += (frame_bytes(files[first + (size_t)i].geo) + 255) & ~(size_t)255; }
    void* d_frames = nullptr;
    if (int rc = mem.get(frames_total + 256, &d_frames)) return rc;
    if (int rc = lep_gpu_memset(g, d_frames, 0, frames_total)) return rc;
    std::vector<lep_segment> dsegs;
    std::vector<uint64_t> offs(1, 0);
    std::vector<uint32_t> lens;
    std::vector<lepbands::File> bfiles((size_t)nf);
    std::vector<lepbands::Segment> bsegs;
    std::vector<lep_huff_image> himgs((size_t)nf);
    lepbatch::OutputArena arena;
    for (int i = 0; i < nf; ++i) {
        Streamed& F = files[first + (size_t)i];
        dev[(size_t)i] = F.geo;
        lepbatch::point_components(dev[(size_t)i].blocks, F.geo.ncomp, (char*)d_frames + frame_off[(size_t)i], [&](int c) { return lepbatch::desc_blocks(F.geo, c); });
        memcpy(&himgs[(size_t)i], &F.plan.image, sizeof(lep_huff_image));
        for (int c = 0; c < 4; ++c) himgs[(size_t)i].blocks[c] = c < F.geo.ncomp ? dev[(size_t)i].blocks[c] : nullptr;
        bfiles[(size_t)i].seg0 = (int)bsegs.size(); bfiles[(size_t)i].nseg = F.nseg;
        uint32_t caps[LEP_MAX_SEGMENTS];
        lepbatch::RecodeSlot slots[LEP_MAX_SEGMENTS];
        for (int q = 0; q < F.nseg; ++q) caps[q] = F.plan.segs[(size_t)q].out_cap;
        lepbatch::place_recode_segments(caps, F.nseg, &arena, slots);
        for (int q = 0; q < F.nseg; ++q) {
            lep_segment s = F.segs[q];
            s.image = i;
            dsegs.push_back(s);
            lens.push_back((uint32_t)F.streams[q].len);
            offs.push_back(offs.back() + ((F.streams[q].len + 255) & ~(size_t)255));
            lep_huff_segment planned;
            memcpy(&planned, &F.plan.segs[(size_t)q], sizeof planned);
            planned.out_cap = slots[q].slot;
            bsegs.emplace_back();
            lepbands::start_segment(&bsegs.back(), i, planned, slots[q].off, q + 1 == F.nseg, slots[q].bound);
        }
    }
    const int nseg = (int)dsegs.size();
    void *d_streams = nullptr, *d_lens = nullptr, *d_arena = nullptr, *d_packed = nullptr, *d_answer = nullptr;
    if (int rc = mem.get((size_t)offs.back() + 256, &d_streams)) return rc;
    if (int rc = mem.get(sizeof(uint32_t) * (size_t)nseg, &d_lens)) return rc;
    {
        std::vector<uint8_t> up((size_t)offs.back());
        int k = 0;
        for (int i = 0; i < nf; ++i) {
            const Streamed& F = files[first + (size_t)i];
            for (int q = 0; q < F.nseg; ++q, ++k) if (F.streams[q].len) memcpy(up.data() + offs[(size_t)k], F.streams[q].data, F.streams[q].len);
        }
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
    std::vector<uint8_t> answer(answer_cap), packed(pack ? arena.bytes : 0), one;

    lep::SessionEnd session{g};
    if (int rc = lep_gpu_decode_rows_begin(g, dev.data(), nf, dsegs.data(), nseg, (const uint8_t*)d_streams, offs.data(), (const uint32_t*)d_lens, nullptr)) return rc;
    session.open = true;
    ++C.stats->sessions;

    // every file's header before the first advance
    for (int i = 0; i < nf; ++i) {
        Streamed& F = files[first + (size_t)i];
        lepbands::File& bf = bfiles[(size_t)i];
        if (F.plan.head.empty()) continue;
        bf.sunk += F.plan.head.size();
        if (C.sink(C.user, F.index, F.plan.head.data(), F.plan.head.size())) bf.gone = true;
    }
    std::vector<lep_decode_progress> prog((size_t)nseg);
    std::vector<lep_huff_segment> launch;
    std::vector<int> which;
    std::vector<uint64_t> src_off;
    int advance = 0;
    for (int running = 1; running > 0;) {
        ++advance;
        for (int i = 0; i < nf; ++i)
            if (!bsegs[(size_t)bfiles[(size_t)i].seg0].complete() && !bsegs[(size_t)bfiles[(size_t)i].seg0].stopped) files[first + (size_t)i].front_last_advance = advance;
        if (int rc = lep_gpu_decode_rows_advance(g, C.band, prog.data(), &running)) return rc;
        ++C.stats->advances;
        // 1. row ranges
        launch.clear(); which.clear(); src_off.clear();
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
                if (!lepbands::band_segment(bsegs[(size_t)k], lepbands::complete_row(bsegs[(size_t)k], prog[(size_t)k], units.vs, d.ncomp), i, &hs)) continue;
                launch.push_back(hs); which.push_back(k); src_off.push_back(hs.out_off);
            }
        }
        if (launch.empty()) continue;
        // 2. one writer launch, 3. pack and two copies (or a copy per segment)
        const int nl = (int)launch.size();
        uint64_t* d_dst_off = (uint64_t*)d_answer;
        lep_huff_end* d_ends = (lep_huff_end*)((char*)d_answer + o_ends);
        uint32_t* d_out_len = (uint32_t*)((char*)d_answer + o_len);
        if (int rc = lep_gpu_huffman_encode_device(g, himgs.data(), nf, launch.data(), nl, (uint8_t*)d_arena, d_out_len, d_ends, nullptr)) return rc;
        ++C.stats->writer_launches;
        if (pack) if (int rc = lep_gpu_pack_device(g, (const uint8_t*)d_arena, src_off.data(), d_out_len, nl, (uint8_t*)d_packed, arena.bytes, d_dst_off, nullptr)) return rc;
        if (int rc = lep_gpu_memcpy_d2h(g, answer.data(), d_answer, answer_cap)) return rc;
        const uint64_t* dst_off = (const uint64_t*)answer.data();
        const lep_huff_end* ends = (const lep_huff_end*)(answer.data() + o_ends);
        const uint32_t* out_len = (const uint32_t*)(answer.data() + o_len);
        if (pack) {
            if (dst_off[nl] > arena.bytes) { lep_gpu_sync(g); return LEP_GPU_ERROR; }
            if (dst_off[nl]) if (int rc = lep_gpu_memcpy_d2h(g, packed.data(), d_packed, (size_t)dst_off[nl])) return rc;
            C.stats->scan_bytes_down += dst_off[nl];
        }
        for (int j = 0; j < nl; ++j) {
            lepbands::Segment& s = bsegs[(size_t)which[(size_t)j]];
            const uint32_t len = std::min(out_len[j], launch[(size_t)j].out_cap);
            const uint8_t* data = nullptr;
            if (pack) data = packed.data() + dst_off[j];
            else {
                one.resize(len);
                if (len) if (int rc = lep_gpu_memcpy_d2h(g, one.data(), (const char*)d_arena + launch[(size_t)j].out_off, len)) return rc;
                C.stats->scan_bytes_down += len;
                data = one.data();
            }
            if (!lepbands::band_written(&s, launch[(size_t)j], data, len, ends[j])) bfiles[(size_t)s.file].declined = true;
        }
        // 4. hand on, in file order
        for (int i = 0; i < nf; ++i) {
            Streamed& F = files[first + (size_t)i];
            lepbands::File& bf = bfiles[(size_t)i];
            const bool had = bf.scan_byte_out;
            lepbands::hand_on(&bf, bsegs, [&](const uint8_t* p, size_t k) { C.piece_with_scan_bytes(); return C.sink(C.user, F.index, p, k) == 0; });
            if (!had && bf.scan_byte_out) F.first_scan_advance = advance;
        }
    }
    session.open = false;
    if (int rc = lep_gpu_decode_rows_end(g)) return rc;
    for (int i = 0; i < nf; ++i) {
        Streamed& F = files[first + (size_t)i];
        C.status[F.index] = finish_file(C, F, bfiles[(size_t)i], bsegs, (const char*)d_frames + frame_off[(size_t)i]);
        if (F.first_scan_advance && F.first_scan_advance < F.front_last_advance) ++C.stats->files_first_scan_byte_before_last_advance;
        F.f.reset();
    }
    return 0;
}
}  // namespace

extern "C" int lep_decompress_batch_stream(lep_gpu* g, const lep_bytes* leps, int n, int band_mcu_rows, lep_batch_sink sink, void* user, int32_t* status,
                                           const lep_batch_options* opt, lep_batch_stream_stats* stats) {
    if (!g) return LEP_GPU_ERROR;
    if (!sink || !status || n < 0 || (n && !leps)) return LEP_ASSERTION_FAILURE;
    lep_batch_stream_stats local;
    if (!stats) stats = &local;
    memset(stats, 0, sizeof *stats);
    Call C{g, band_mcu_rows, sink, user, status, stats, Clock::now()};
    int session_files = 64;
    if (const char* e = getenv("LEP_STREAM_SESSION_FILES")) if (atoi(e) > 0) session_files = atoi(e);
    std::vector<Streamed> files;
    std::vector<int> whole;
    for (int i = 0; i < n; ++i) {
        status[i] = LEP_CODING_ERROR;
        lep_file* f = nullptr;
        Streamed F;
        if (lep_file_open(leps[i].data, leps[i].len, &f) == 0) {
            F.f.reset(f);
            if (lep::streams_in_session(f, leps[i].data, leps[i].len, &F.plan, F.segs, F.streams, &F.nseg) &&
                lep_file_describe_into(f, nullptr, (size_t)-1, &F.geo) == 0) {
                F.index = i;
                files.push_back(std::move(F));
                continue;
            }
        }
        whole.push_back(i);   // (a file that does not parse gets its exit code from lep_decompress_batch)
    }
    stats->files_streamed = (int)files.size();
    stats->files_whole = (int)whole.size();
    int rc = 0;
    for (size_t first = 0; first < files.size() && !rc;) {
        size_t last = first;
        int segs = 0;
        while (last < files.size() && (int)(last - first) < session_files && segs + files[last].nseg <= kSessionSegments) segs += files[last++].nseg;
        rc = run_session(C, files, first, last);
        first = last;
    }
    files.clear();
    if (!rc && !whole.empty()) {
        std::vector<lep_bytes> in(whole.size()), outs(whole.size(), lep_bytes{nullptr, 0, 0});
        std::vector<int32_t> st(whole.size(), LEP_CODING_ERROR);
        for (size_t k = 0; k < whole.size(); ++k) in[k] = leps[whole[k]];
        rc = lep_decompress_batch(g, in.data(), (int)whole.size(), outs.data(), st.data(), opt, nullptr);
        for (size_t k = 0; k < whole.size(); ++k) {
            status[whole[k]] = rc ? rc : st[k];
            if (!rc && st[k] == 0 && outs[k].data) {
                C.piece_with_scan_bytes();
                if (sink(user, whole[k], outs[k].data, outs[k].len)) status[whole[k]] = LEP_OS_ERROR;
            }
            if (outs[k].data) lep_free(outs[k].data);
        }
    }
    stats->wall_s = std::chrono::duration<double>(Clock::now() - C.t0).count();
    return rc;
}
