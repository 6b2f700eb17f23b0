// The session loop of lep_decompress_batch_ranges (lepton_amd/csrc/lep_batch_ranges.cc) stepped on the CPU for one file and one range: the
// plan is the library's (lep_file_range_plan), the bookkeeping the product's (lep_stream_bands.h, lep_range_bands.h), the decode is faked
// -- after every advance a running segment stands the band's height further behind its first row, over a frame that is already whole, and
// a retired segment stands still --, every band is written by the emulated lane scan writer of core_emu.cc (the wavefront form where the
// lane form does not take a segment) into the segment's slot, and the windowed pack is lep_pack.h's window_len and copy_run, lane by
// lane, from the slot to the answer.  The finish's checks and tail are the library's (C ABI).
#include "core_emu.cc"

#include "../../lepton_amd/csrc/lep_pack.h"
#include "../../lepton_amd/csrc/lep_range_bands.h"

struct emu_range_report {
    int32_t advances, nseg;
    int32_t touched[LEP_MAX_SEGMENTS];          // 1: given to the session
    int32_t retired[LEP_MAX_SEGMENTS];          // 1: retired with its window served
    int32_t retire_advance[LEP_MAX_SEGMENTS];   // the advance behind which it was retired (0: never)
    int32_t rows_coded[LEP_MAX_SEGMENTS];       // planned rows written when it finished or was retired
    uint64_t written[LEP_MAX_SEGMENTS];         // bytes its writer appended
    uint64_t kept[LEP_MAX_SEGMENTS];            // bytes of them that were kept
    uint64_t host_bytes;                        // bytes lepbands::Segment::bytes held at the end, all segments (must be 0)
};

// Cumulative byte counts of segment q written one MCU row per band by the same coder: cum[k] = bytes after k + 1 bands.  Returns the bands.
extern "C" int emu_segment_row_bytes(lep_file* f, int q, uint64_t* cum, int cap) {
    lep_huff_image img;
    lep_huff_segment planned[LEP_MAX_SEGMENTS];
    int nseg = 0, ok = 0;
    if (lep_file_recode_plan(f, &img, planned, &nseg, &ok) || !ok || q >= nseg) return -1;
    lepbands::Segment s;
    lepbands::start_segment(&s, 0, planned[q], 0, q + 1 == nseg);
    std::vector<uint8_t> slot((size_t)planned[q].out_cap + 8);
    lep_image_desc geo;
    if (lep_file_describe_into(f, nullptr, (size_t)-1, &geo)) return -1;
    const int step = lepbands::row_units(geo, img).per_mcu_row;   // planned rows per MCU row
    int rows = 0;
    for (int row = s.row0; row < s.row1 && rows < cap; row += step, ++rows) {
        lep_huff_segment hs;
        if (!lepbands::band_segment(s, std::min(row + step, s.row1), 0, &hs)) return -2;
        uint32_t n = 0;
        lep_huff_end end;
        memset(&end, 0, sizeof end);
        if (emu_huffman_encode_segment_simt(&img, &hs, slot.data() + hs.out_off, &n, &end) == 1) emu_huffman_encode_segment(&img, &hs, slot.data() + hs.out_off, &n, &end);
        if (!lepbands::band_counted(&s, hs, n, end)) return -3;
        cum[rows] = s.written;
        if (s.complete()) { ++rows; break; }
    }
    return rows;
}

// 0, or the status the call would give the file; LEP_GPU_PATH_DECLINED: the whole-file path would take it.  answer: cap bytes, *answer_len.
extern "C" int emu_range_bands(lep_file* f, const uint8_t* lepdata, size_t len, uint64_t first, uint64_t length, int band, uint8_t* answer, size_t cap, size_t* answer_len,
                               emu_range_report* rep) {
    memset(rep, 0, sizeof *rep);
    lep_range_plan rp;
    if (int rc = lep_file_range_plan(lepdata, len, first, length, &rp)) return rc;
    if (!rp.in_session || !rp.sizes_known) return -1;
    lep_huff_image img;
    lep_huff_segment planned[LEP_MAX_SEGMENTS];
    int nseg = 0, ok = 0;
    if (int rc = lep_file_recode_plan(f, &img, planned, &nseg, &ok)) return rc;
    if (!ok || nseg != rp.nseg) return -1;
    rep->nseg = nseg;
    const uint8_t* head = nullptr;
    size_t head_len = 0;
    if (int rc = lep_file_recode_head(f, &head, &head_len)) return rc;
    if (head_len != rp.head_len || rp.length > cap) return -4;
    std::vector<uint8_t> out((size_t)rp.length, 0);
    if (rp.head_bytes) memcpy(out.data(), head + rp.first, (size_t)rp.head_bytes);
    std::vector<leprange::Touched> touched;
    leprange::touched_of(rp, &touched);
    const int nt = (int)touched.size();
    std::vector<lepbands::Segment> segs((size_t)nt);
    std::vector<std::vector<uint8_t>> slot((size_t)nt);
    std::vector<int> stands((size_t)nt);
    for (int i = 0; i < nt; ++i) {
        const int q = touched[(size_t)i].q;
        rep->touched[q] = 1;
        slot[(size_t)i].assign((size_t)planned[q].out_cap + 8, 0xEE);
        lepbands::start_segment(&segs[(size_t)i], 0, planned[q], 0, q + 1 == nseg);
        stands[(size_t)i] = segs[(size_t)i].row0;
    }
    lep_image_desc geo;
    if (int rc = lep_file_describe_into(f, nullptr, (size_t)-1, &geo)) return rc;
    const lepbands::RowUnits units = lepbands::row_units(geo, img);
    bool declined = false;
    leprange::Schedule bands(band);
    for (int live = nt; live > 0;) {
        ++rep->advances;
        const int h = bands.height() * units.per_mcu_row;   // (planned rows of one advance)
        live = 0;
        for (int i = 0; i < nt; ++i) {
            lepbands::Segment& s = segs[(size_t)i];
            leprange::Touched& t = touched[(size_t)i];
            if (t.settled) continue;
            stands[(size_t)i] = std::min(s.row1, stands[(size_t)i] + h);   // the faked decode
            lep_decode_progress p;
            memset(&p, 0, sizeof p);
            p.status = stands[(size_t)i] >= s.row1 ? 0 : -1;
            for (int c = 0; c < img.ncomp && c < LEP_MAX_COMPONENTS; ++c) p.rows_done[c] = stands[(size_t)i] * units.vs[c];
            lep_huff_segment hs;
            if (!declined && lepbands::band_segment(s, lepbands::complete_row(s, p, units.vs, img.ncomp), 0, &hs)) {
                uint8_t* w = slot[(size_t)i].data() + (hs.out_off - s.slot_off);
                uint32_t n = 0, sk = 0, tk = 0;
                lep_huff_end end;
                memset(&end, 0, sizeof end);
                if (emu_huffman_encode_segment_simt(&img, &hs, w, &n, &end) == 1) emu_huffman_encode_segment(&img, &hs, w, &n, &end);
                leprange::band_window(t, s.written, hs.out_cap, &sk, &tk);
                const uint32_t keep = leppack::window_len(n, sk, tk);   // (the offsets kernel, from the writer's count)
                const uint64_t at = leprange::band_out_at(t, s.written);
                if (keep) {
                    if (at + keep > out.size()) return -5;
                    for (uint32_t lane = 0; lane < 64; ++lane) leppack::copy_run(w + sk, out.data() + at, keep, lane);
                    t.kept += keep;
                }
                if (!lepbands::band_counted(&s, hs, n, end)) declined = true;
            }
            const bool runs = p.status == -1;
            const bool served = !s.complete() && leprange::window_reached(t, s.written);
            if (!runs || served || s.complete() || declined) {
                t.settled = true;
                rep->rows_coded[t.q] = s.coded - s.row0;
                if (served && !declined) { t.retired = true; rep->retired[t.q] = 1; rep->retire_advance[t.q] = rep->advances; }
            } else ++live;
        }
    }
    for (int i = 0; i < nt; ++i) {
        const int q = touched[(size_t)i].q;
        rep->written[q] = segs[(size_t)i].written;
        rep->kept[q] = touched[(size_t)i].kept;
        rep->host_bytes += segs[(size_t)i].bytes.size();
        for (size_t k = segs[(size_t)i].slot_cap; k < slot[(size_t)i].size(); ++k) if (slot[(size_t)i][k] != 0xEE) return -2;   // nothing behind a slot was written
    }
    if (declined) return LEP_GPU_PATH_DECLINED;
    int rc = leprange::finish(
        rp, touched, segs.data(),
        [&](int q, const lep_huff_end& end, uint64_t bytes, bool last_of_file) { return lep_file_recode_segment_end(f, q, &end, bytes, last_of_file ? 1 : 0); },
        [&](uint64_t bytes_in_front, std::vector<uint8_t>* tail, uint64_t* at) {
            lep_bytes tb = {nullptr, 0, 0};
            if (lep_file_recode_tail(f, bytes_in_front, &tb, at) == 0) { tail->assign(tb.data, tb.data + tb.len); lep_free(tb.data); }
        },
        &out);
    if (rc) return rc;
    memcpy(answer, out.data(), out.size());
    *answer_len = out.size();
    return 0;
}
