// prog_simt_driver.h -- TEST ONLY: the scans of one image as lep_gpu_huffman_progressive_encode_device routes them, every pass of
// lep_huffprog_simt.h one emulated wavefront after the other.  What the lane form takes, and its descriptors, region and unit count,
// come from prog_simt_plan -- the launch code's own plan; the wavefront form (lep_huffprog.h) writes the rest.  Included by core_emu.cc
// and prog_simt_rst_emu.cc, which the tests build as separate libraries.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../lepton_amd/csrc/lep_huffprog_simt.h"

// taken[i]: 0 wavefront form, 1 lane form (or `sequential`), 2 lane form with restart intervals.  rst_on: the lane form takes scans with a
// restart interval.  region_bytes > 0 stands in for the plan's region size.  sequential: who writes a scan of a sequential frame (returns
// its out_len); nullptr: such a scan is refused with 2.  Unit arrays and region are filled with garbage first, the marker maps cleared
// as the zero kernel clears them.  *guards_intact: the words in front of and behind the region, and behind the unit arrays, still hold
// what they were filled with.
inline int emu_prog_simt_drive(const lep_huffprog_image* img, const lep_huffprog_scan* scans, int nscan, uint8_t* out, uint32_t* corr, uint32_t* out_len, int32_t* taken,
                               uint64_t region_bytes, bool rst_on, uint32_t (*sequential)(const lephuff::ProgImage*, const lephuff::ProgScan&, uint8_t*), int32_t* guards_intact) {
    static lephuff::ProgSimtShared sh;
    static lephuff::ProgShared shw;
    const lephuff::ProgImage* im = reinterpret_cast<const lephuff::ProgImage*>(img);
    std::vector<lephuff::ProgScan> sv((size_t)nscan);
    memcpy(sv.data(), scans, sizeof(lephuff::ProgScan) * (size_t)nscan);
    std::vector<uint32_t> file_bound((size_t)nscan);
    for (int i = 0; i < nscan; ++i) {
        file_bound[(size_t)i] = sv[(size_t)i].pad;   // (lep_huffprog_scan.file_bound)
        sv[(size_t)i].pad = 0; sv[(size_t)i].image = 0; taken[i] = 0;
        if (lephuff::prog_is_sequential(sv[(size_t)i]) && !sequential) return 2;
    }
    for (int i = 0; i < nscan; ++i)
        if (lephuff::prog_is_sequential(sv[(size_t)i])) { out_len[i] = sequential(im, sv[(size_t)i], out); taken[i] = 1; }
    lephuff::ProgSimtPlan plan;
    lephuff::prog_simt_plan(im, 1, sv.data(), nscan, file_bound.data(), true, rst_on, &plan, region_bytes);
    std::vector<lephuff::ProgSimtScan>& ps = plan.ps;
    for (const auto& e : ps) taken[e.scan] = e.rsti ? 2 : 1;
    const size_t guard = 64;   // dwords
    const size_t unit_words = plan.nunits * (size_t)lephuff::prog_simt_unit_words(plan.intervals);
    std::vector<uint32_t> words(unit_words + guard, 0xdeadbeefu);
    std::vector<uint32_t> scratch(guard + plan.scratch_bytes / 4 + guard, 0xa5a5a5a5u);   // (garbage: the clearing pass has to do its work)
    uint8_t* scb = reinterpret_cast<uint8_t*>(scratch.data() + guard);
    lephuff::ProgSimtUnits U;
    U.set(words.data(), plan.nunits);
    for (auto& e : ps) for (uint32_t f = 0; f < e.nunits; f += 64) lephuff::prog_simt_units<false>(im, sv.data(), &e, &sh, U, scb, f);
    for (auto& e : ps) lephuff::prog_simt_place(sv.data(), &e, U);
    for (const auto& r : plan.regions) lephuff::prog_simt_assign(r, ps.data());
    for (auto& e : ps) {   // (lep_huffprog_simt_zero_kernel)
        const uint64_t need16 = std::min<uint64_t>(((uint64_t)e.total_bits + 7) / 8 / 16 + 2, e.buf_bytes / 16);
        memset(scb + e.buf_off, 0, (size_t)need16 * 16);
        memset(scb + e.buf_off + e.buf_bytes, 0, e.map_bytes);
    }
    for (auto& e : ps) for (uint32_t f = 0; f < e.nunits; f += 64) lephuff::prog_simt_units<true>(im, sv.data(), &e, &sh, U, scb, f);
    for (auto& e : ps) lephuff::prog_simt_stuff(im, sv.data(), e, scb, out, out_len);
    for (int i = 0; i < nscan; ++i)
        if (!taken[i]) { lephuff::ProgWave w; out_len[i] = w.run_scan(im, &sv[(size_t)i], &shw, out, corr); }
    bool intact = true;
    for (size_t k = 0; k < guard; ++k) intact = intact && scratch[k] == 0xa5a5a5a5u && scratch[guard + plan.scratch_bytes / 4 + k] == 0xa5a5a5a5u && words[unit_words + k] == 0xdeadbeefu;
    *guards_intact = intact ? 1 : 0;
    return 0;
}
