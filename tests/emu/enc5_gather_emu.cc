// enc5_gather_emu.cc -- TEST ONLY: the split-phase encoder (lepton_amd/csrc/lep_enc5.h) stepped as 64-lane loop emulations, as
// core_emu.cc's encode_segment_v5 steps it -- count -> plan -> emit -> bucket -> fold (every chain) -> gather -> write -- but
// handing back the WHOLE bin list, the poisoned room behind the bins included, so that the staging of gather's bins
// (Walk5::put_bin / drain / flush_bin) can be held against the form before (-DLEP_ENC5_GATHER_ROW_FLUSH=0) half word for half word.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
#define LEP_DEV inline
#include "../../lepton_amd/csrc/lep_derive.h"
#include "../../lepton_amd/csrc/lep_enc3.h"
#include "../../lepton_amd/csrc/lep_enc5.h"

using namespace lepdev;

static const uint16_t kPoison = 0xA5A5;

template <int NW>
static int encode(const lep_image_desc* d, int y0, int y1, int is_last, int nparts, uint8_t* out, uint32_t cap, uint32_t* len, uint32_t* nbins,
                  uint16_t* list_out, uint32_t list_cap, uint32_t* list_len) {
    using namespace lep5;
    ImageDev img;
    int rc = derive_image(*d, &img, true);
    if (rc) return rc;
    std::vector<NSum> ns(img.ns_total);
    SegDev seg;
    seg.image = 0; seg.y0 = y0; seg.y1 = y1; seg.is_last = is_last; seg.stream_off = 0; seg.stream_cap = cap; seg.slot = 0;
    static Walk5Shared wsh;
    static FoldShared fsh;
    static BucketShared bsh;
    static SegPlan5 plan;
    std::vector<uint32_t> counts(kCountWords, 0);
    {
        Walk5<kCount, NW> w;
        memset(ns.data(), 0, ns.size() * sizeof(NSum));
        w.run(&img, seg, ns.data(), &wsh, &plan, nullptr, nullptr);
        export_counts(w, &wsh, counts.data());
    }
    plan_segment(counts.data(), &plan);
    std::vector<uint8_t> arena(plan.arena_bytes + 64, 0xA5);
    std::vector<uint16_t> binlist(plan.bins_cap + 64, kPoison);
    {
        Walk5<kEmit, NW> w;
        memset(ns.data(), 0, ns.size() * sizeof(NSum));
        rc = w.run(&img, seg, ns.data(), &wsh, &plan, arena.data(), nullptr, 0, 0, nparts);
        if (rc) return rc;
    }
    bucket_wave(&plan, arena.data(), &bsh);
    std::vector<uint32_t> thresh(kThreshWords, kBranchInit);
    for (int ci = 0; ci < 2; ++ci) {
        for (int row = 0; row < kRows; ++row)
            for (int k = 0; k < kClasses; ++k) {
                const int sid = stream_id(ci, row, k);
                if (!plan.cnt[sid]) continue;
                if (row < 63) fold_coef_wave(&plan, arena.data(), 0, 1, sid, &fsh);
                else fold_thresh_wave(&plan, arena.data(), thresh.data(), 0, 1, sid, ci, &fsh);
            }
        fold_sign_wave(&plan, arena.data(), 0, 1, ci, &fsh);
        for (int b = 0; b < 10; ++b) fold_nz_wave(&plan, arena.data(), 0, 1, ci, b, &fsh);
        for (int v = 0; v < 2; ++v) for (int e = 0; e < 8; ++e) fold_edgenz_wave(&plan, arena.data(), 0, 1, ci, v, e, &fsh);
    }
    for (int a = 0; a < 12; ++a) fold_dc_wave(&plan, arena.data(), 0, 1, a, &fsh);
    for (int part = 0; part < nparts; ++part) {   // (every part: a walker of its own, as on the GPU)
        Walk5<kGather, NW> w;
        memset(ns.data(), 0, ns.size() * sizeof(NSum));
        rc = w.run(&img, seg, ns.data(), &wsh, &plan, arena.data(), binlist.data(), 0, part, nparts);
        if (rc) return rc;
        if (w.nbins > plan.bins_cap) return 1003;
        plan.nbins = w.nbins;
    }
    *nbins = plan.nbins;
    *list_len = (uint32_t)binlist.size();
    memcpy(list_out, binlist.data(), 2 * (binlist.size() < list_cap ? binlist.size() : (size_t)list_cap));
    uint32_t slen = 0;
    int32_t status = 0;
    for (int part = 0; part < nparts; ++part) write_wave(&plan, binlist.data(), &seg, 0, 1, out, &slen, &status, arena.data(), part, nparts);
    *len = slen;
    return status == 100 ? LEP_BUFFER_TOO_SMALL : status;
}

// waves: 1 = one wavefront walks the whole block, 2 = the walks' two halves apart; nparts: gather and write in this many parts.
// list_out takes the bin list AND the room behind it as the passes left it (list_len half words, poisoned with 0xA5A5 before gather)
extern "C" int emu_enc5_gather(const lep_image_desc* d, int y0, int y1, int is_last, int waves, int nparts, uint8_t* out, uint32_t cap, uint32_t* len,
                               uint32_t* nbins, uint16_t* list_out, uint32_t list_cap, uint32_t* list_len) {
    return waves == 2 ? encode<2>(d, y0, y1, is_last, nparts, out, cap, len, nbins, list_out, list_cap, list_len)
                      : encode<1>(d, y0, y1, is_last, nparts, out, cap, len, nbins, list_out, list_cap, list_len);
}
extern "C" int emu_enc5_gather_knobs() { return LEP_ENC5_GATHER_ROW_FLUSH; }
