// dec_rows_emu.cc -- TEST ONLY: core_emu.cc plus a driver that steps the resumable decoder (lep_dec4.h, Dec4WaveT::run_rows) band after
// band over ONE resume record, the way lep_gpu_decode_rows_advance launches lep_decode_v4_rows_kernel: the model, the summary rings, the
// record and the saved LDS Branches persist between bands, everything else (the wave object, Dec4Shared) is made anew for every band.
#include "core_emu.cc"

#include "../../include/lepton_mi355x.h"

// Decodes segment [y0, y1) of `d` from `in` in bands of band_mcu_rows MCU rows (<= 0: one band to the end).  progress_out[k] receives
// the record as lep_gpu_decode_rows_advance reports it after band k (k < max_bands).  Returns the number of bands run, or -1 - that
// number when the segment was still running after max_bands of them; *bins = the bins counted.  The segment's exit code is the last
// record's status.  after_band (optional) is called behind every band with the band's index: the frame is the caller's memory, to be looked at there.
typedef void (*emu_after_band)(void* user, int band);
extern "C" int emu_decode_segment_v4_rows_watched(const lep_image_desc* d, int y0, int y1, int is_last, const uint8_t* in, uint32_t len, int band_mcu_rows,
                                                  lep_decode_progress* progress_out, int max_bands, uint32_t* bins, emu_after_band after_band, void* user) {
    ImageDev img;
    if (int rc = derive_image(*d, &img, false)) return -1000 - rc;
    std::vector<lep3::U4> model(lep3::kModelWords / 4, lep3::U4{kBranchInit, kBranchInit, kBranchInit, kBranchInit});
    std::vector<NSum> ns(img.ns_total);
    memset(ns.data(), 0, ns.size() * sizeof(NSum));
    SegDev seg;
    seg.image = 0; seg.y0 = y0; seg.y1 = y1; seg.is_last = is_last; seg.stream_off = 0; seg.stream_cap = 0; seg.slot = 0;
    PaddedStream ps(in, len);
    lep4::Dec4Resume rec;
    memset(&rec, 0, sizeof rec);   // all zero = fresh, as lep_gpu_decode_rows_begin clears it
    std::vector<uint32_t> lds_save(lep3::kSignWords + lep3::kResDcWords, 0xdeadbeefu);
    int bands = 0;
    while (rec.state == lep4::kRowsFresh || rec.state == lep4::kRowsRunning) {
        if (bands >= max_bands) return -1 - bands;
        static lep4::Dec4Shared sh;
        memset(&sh, 0xa5, sizeof sh);   // nothing of the band before may be relied on
        lep4::Dec4Wave w;
        w.run_rows(&img, seg, reinterpret_cast<uint32_t*>(model.data()), ns.data(), &sh, ps.p, len, &rec, lds_save.data(), band_mcu_rows);
        lep_decode_progress& p = progress_out[bands++];
        const bool failed = rec.state == lep4::kRowsFailed;
        p.status = rec.state == lep4::kRowsFinished ? 0 : (failed ? rec.code : -1);
        for (int c = 0; c < LEP_MAX_COMPONENTS; ++c) p.rows_done[c] = rec.rows_done[c];
        p.fail_component = failed ? rec.fail_component : -1; p.fail_y = failed ? rec.fail_y : -1; p.fail_x = failed ? rec.fail_x : -1;
        p.bins = rec.nbins;
        if (after_band) after_band(user, bands - 1);
    }
    if (bins) *bins = rec.nbins;
    return bands;
}
extern "C" int emu_decode_segment_v4_rows(const lep_image_desc* d, int y0, int y1, int is_last, const uint8_t* in, uint32_t len, int band_mcu_rows,
                                          lep_decode_progress* progress_out, int max_bands, uint32_t* bins) {
    return emu_decode_segment_v4_rows_watched(d, y0, y1, is_last, in, len, band_mcu_rows, progress_out, max_bands, bins, nullptr, nullptr);
}
