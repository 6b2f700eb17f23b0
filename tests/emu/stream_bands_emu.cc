// The band loop of lep_decompress_batch_stream (lepton_amd/csrc/lep_batch_stream.cc) stepped on the CPU for one file: the bookkeeping is
// the product's (lep_stream_bands.h), the decode is faked -- after advance k every segment stands k x band MCU rows behind its first row,
// over a frame that is already whole --, and every band is written by the emulated lane scan writer of core_emu.cc (the wavefront form
// where the lane form does not take a segment).  Head, finish and the host re-coder are the library's (C ABI).
#include "core_emu.cc"

#include "../../lepton_amd/csrc/lep_stream_bands.h"

// seg: -1 the header, -2 the tail behind the scan, otherwise the thread segment the bytes belong to; advance: how many advances were made
typedef int (*emu_piece_fn)(void* user, int seg, int advance, const uint8_t* data, size_t len);

// shrink_seg >= 0: that segment's slot is shrink_cap bytes (the writer outgrows it).  *declined: the host re-coder finished the file.
extern "C" int emu_stream_bands(lep_file* f, int band, int shrink_seg, uint32_t shrink_cap, emu_piece_fn piece, void* user, int32_t* declined, int32_t* advances) {
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
        if (q == shrink_seg) planned[q].out_cap = shrink_cap;
        slot[(size_t)q].assign((size_t)planned[q].out_cap + 8, 0xEE);
        lepbands::start_segment(&segs[(size_t)q], 0, planned[q], 0);
    }
    int advance = 0;
    bf.sunk += head_len;
    if (head_len && piece(user, -1, advance, head, head_len)) bf.gone = true;
    int vs[LEP_MAX_COMPONENTS] = {1, 1, 1};   // from the geometry, as the product derives it; the faked decode counts rows the same way
    lep_image_desc geo;
    if (int rc = lep_file_describe_into(f, nullptr, (size_t)-1, &geo)) return rc;
    lepbands::block_rows_per_mcu_row(geo, vs);
    for (int c = 0; c < img.ncomp && c < LEP_MAX_COMPONENTS; ++c) if (vs[c] != img.vs[c]) return -3;   // ... and the writer's plan agrees
    for (bool running = true; running;) {
        ++advance;
        running = false;
        for (int q = 0; q < nseg; ++q) {
            lepbands::Segment& s = segs[(size_t)q];
            const int stands = band > 0 ? std::min(s.row1, s.row0 + advance * band) : s.row1;   // the faked decode
            lep_decode_progress p;
            memset(&p, 0, sizeof p);
            p.status = stands >= s.row1 ? 0 : -1;
            for (int c = 0; c < img.ncomp && c < LEP_MAX_COMPONENTS; ++c) p.rows_done[c] = stands * vs[c];
            if (p.status < 0) running = true;
            lep_huff_segment hs;
            if (!bf.writes() || !lepbands::band_segment(s, lepbands::complete_row(s, p, vs, img.ncomp), 0, &hs)) continue;
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
