// The band loop of lep_decompress_batch_stream (lepton_amd/csrc/lep_batch_stream.cc) stepped on the CPU for one file of the layouts
// tests/emu/stream_bands_emu.cc does not reach: one-component files (the writer's rows are block rows), -startbyte / -trunc slices and files
// cut inside their scan.  The bookkeeping is the product's (lep_stream_bands.h) -- the row units too: lepbands::row_units says how many
// block rows of a component a planned row holds and how many planned rows a band of one MCU row adds; nothing here knows a layout.  The
// decode is faked in the decoder's own units: after advance k every segment stands k x band MCU rows behind the MCU row it starts in, and
// rows_done counts frame block rows.  Every band is written by the emulated lane scan writer of core_emu.cc (the wavefront form where the
// lane form does not take a segment).  Head, finish and the host re-coder are the library's (C ABI).
#include "core_emu.cc"

#include "../../lepton_amd/csrc/lep_stream_bands.h"

// seg: -1 the header, -2 the tail behind the scan, otherwise the thread segment the bytes belong to; advance: how many advances were made
typedef int (*emu_piece_fn)(void* user, int seg, int advance, const uint8_t* data, size_t len);

// planned rows (lep_huff_segment.mcu_row0 / mcu_row1) that one MCU row of a band adds, as the product derives it
extern "C" int emu_planned_rows_per_mcu_row(lep_file* f) {
    lep_huff_image img;
    lep_huff_segment planned[LEP_MAX_SEGMENTS];
    int nseg = 0, ok = 0;
    lep_image_desc geo;
    if (lep_file_recode_plan(f, &img, planned, &nseg, &ok) || !ok || lep_file_describe_into(f, nullptr, (size_t)-1, &geo)) return -1;
    return lepbands::row_units(geo, img).per_mcu_row;
}

// shrink_seg >= 0: that segment's SLOT is shrink_cap bytes, its byte bound stays the plan's (a slot smaller than the bound: the writer
// outgrows it).  grow_last > 0: the last segment's byte bound AND slot are the plan's + grow_last bytes -- a cut that is met with the
// bound not reached.  *declined: the host re-coder finished the file.
extern "C" int emu_stream_layouts(lep_file* f, int band, int shrink_seg, uint32_t shrink_cap, uint32_t grow_last, emu_piece_fn piece, void* user, int32_t* declined,
                                  int32_t* advances) {
    lep_huff_image img;
    lep_huff_segment planned[LEP_MAX_SEGMENTS];
    int nseg = 0, ok = 0;
    if (int rc = lep_file_recode_plan(f, &img, planned, &nseg, &ok)) return rc;
    if (!ok || nseg <= 0) return -1;
    const uint8_t* head = nullptr;
    size_t head_len = 0;
    if (int rc = lep_file_recode_head(f, &head, &head_len)) return rc;
    std::vector<lepbands::Segment> segs((size_t)nseg);
    std::vector<std::vector<uint8_t>> slot((size_t)nseg);
    lepbands::File bf;
    bf.seg0 = 0; bf.nseg = nseg;
    for (int q = 0; q < nseg; ++q) {
        uint32_t bound = planned[q].out_cap;
        if (q + 1 == nseg && grow_last) planned[q].out_cap = bound = bound + grow_last;
        if (q == shrink_seg) planned[q].out_cap = shrink_cap;
        slot[(size_t)q].assign((size_t)planned[q].out_cap + 8, 0xEE);
        lepbands::start_segment(&segs[(size_t)q], 0, planned[q], 0, q + 1 == nseg, bound);
    }
    int advance = 0;
    bf.sunk += head_len;
    if (head_len && piece(user, -1, advance, head, head_len)) bf.gone = true;
    lep_image_desc geo;
    if (int rc = lep_file_describe_into(f, nullptr, (size_t)-1, &geo)) return rc;
    const lepbands::RowUnits units = lepbands::row_units(geo, img);
    int frame_vs[LEP_MAX_COMPONENTS] = {1, 1, 1};   // what the decoder's rows_done counts: frame block rows per MCU row
    lepbands::block_rows_per_mcu_row(geo, frame_vs);
    for (bool running = true; running;) {
        ++advance;
        running = false;
        for (int q = 0; q < nseg; ++q) {
            lepbands::Segment& s = segs[(size_t)q];
            // the faked decode: MCU rows [first, first + advance x band) of the segment are in the frame
            const int first = s.row0 / units.per_mcu_row, last = (s.row1 + units.per_mcu_row - 1) / units.per_mcu_row;
            const int stands = band > 0 ? std::min(last, first + advance * band) : last;
            lep_decode_progress p;
            memset(&p, 0, sizeof p);
            p.status = stands >= last ? 0 : -1;
            for (int c = 0; c < img.ncomp && c < LEP_MAX_COMPONENTS; ++c) p.rows_done[c] = stands * frame_vs[c];
            if (p.status < 0) running = true;
            lep_huff_segment hs;
            if (!bf.writes() || !lepbands::band_segment(s, lepbands::complete_row(s, p, units.vs, img.ncomp), 0, &hs)) continue;
            if (hs.mcu_row1 > s.row1 || hs.mcu_row0 < s.row0 || hs.out_off - s.slot_off + hs.out_cap > s.slot_cap) return -4;
            uint8_t* out = slot[(size_t)q].data() + (hs.out_off - s.slot_off);
            uint32_t n = 0;
            lep_huff_end end;
            memset(&end, 0, sizeof end);
            if (emu_huffman_encode_segment_simt(&img, &hs, out, &n, &end) == 1) emu_huffman_encode_segment(&img, &hs, out, &n, &end);
            if (!lepbands::band_written(&s, hs, out, n, end)) bf.declined = true;
        }
        lepbands::hand_on(&bf, segs, [&](const uint8_t* p, size_t k) {
            return piece(user, bf.front, advance, p, k) == 0;
        });
    }
    *advances = advance;
    *declined = bf.declined ? 1 : 0;
    for (int q = 0; q < nseg; ++q)   // nothing behind a slot was written
        for (size_t k = segs[(size_t)q].slot_cap; k < slot[(size_t)q].size(); ++k) if (slot[(size_t)q][k] != 0xEE) return -2;
    if (bf.gone) return LEP_OS_ERROR;
    lep_bytes jpg = {nullptr, 0, 0};
    int rc = LEP_GPU_PATH_DECLINED;   // (any failure of the finish: the host re-coder decides, as in lep_batch_stream.cc)
    if (!bf.declined) {
        std::vector<lep_bytes> sb((size_t)nseg);
        std::vector<lep_huff_end> ends((size_t)nseg);
        for (int q = 0; q < nseg; ++q) { sb[(size_t)q] = {segs[(size_t)q].bytes.data(), segs[(size_t)q].bytes.size(), segs[(size_t)q].bytes.size()}; ends[(size_t)q] = segs[(size_t)q].end; }
        rc = lep_file_recode_finish(f, sb.data(), ends.data(), nseg, &jpg);
        if (rc) *declined = 1;
    }
    if (rc) rc = lep_file_recode(f, &jpg);
    if (rc) return rc;
    rc = lepbands::front_of(bf, segs, head, head_len, jpg.data, jpg.len) ? 0 : LEP_ASSERTION_FAILURE;
    if (!rc && jpg.len > bf.sunk && piece(user, -2, advance, jpg.data + bf.sunk, jpg.len - (size_t)bf.sunk)) rc = LEP_OS_ERROR;
    lep_free(jpg.data);
    return rc;
}
