// prog_simt_rst_emu.cc -- TEST ONLY: lep_huffprog_simt.h (progressive scans, with a restart interval and without, written with one lane per
// run of blocks) compiled with g++ as a lane-loop emulation (lep_wave.h), with the launch code's routing around it.  Never linked into the product.
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
#define LEP_DEV inline
#include "../../lepton_amd/csrc/lep_derive.h"
#include "../../lepton_amd/csrc/lep_huffprog_simt.h"

// The scans of one image as lep_gpu_huffman_progressive_encode_device routes them: lep_huffprog_simt.h's form where it takes the scan
// (one with a restart interval: where rst_on says so), the wavefront form (lep_huffprog.h) for the rest; all lane-form scans share one
// region of bit buffers.  Every pass one emulated wavefront after the other, unit arrays and region filled with garbage first.
// taken[i]: 0 wavefront form, 1 lane form, 2 lane form with restart intervals.  region_bytes > 0 stands in for the launch code's region size.
// *guards_intact: the words in front of and behind the region (and behind the unit arrays) still hold what they were filled with.
extern "C" int emu_huffman_progressive_encode_lanes(const lep_huffprog_image* img, const lep_huffprog_scan* scans, int nscan, uint8_t* out, uint32_t* corr, uint32_t* out_len,
                                                    int32_t* taken, uint64_t region_bytes, int rst_on, int32_t* guards_intact) {
    static lephuff::ProgSimtShared sh;
    static lephuff::ProgShared shw;
    const lephuff::ProgImage* im = reinterpret_cast<const lephuff::ProgImage*>(img);
    std::vector<lephuff::ProgScan> sv((size_t)nscan);
    memcpy(sv.data(), scans, sizeof(lephuff::ProgScan) * (size_t)nscan);
    std::vector<lephuff::ProgSimtScan> ps;
    size_t nunits = 0;
    uint64_t sum_cap = 0, bound = 0;
    bool maps = false;
    for (int i = 0; i < nscan; ++i) {
        bound = std::max<uint64_t>(bound, sv[(size_t)i].pad);   // (lep_huffprog_scan.file_bound)
        sv[(size_t)i].pad = 0; sv[(size_t)i].image = 0; taken[i] = 0;
        if (lephuff::prog_is_sequential(sv[(size_t)i])) return 2;   // (scans of sequential frames are not this file's subject)
        uint32_t nb = 0, nu = 0, interval = 0;
        if (!lephuff::prog_simt_takes(*im, sv[(size_t)i], &nb, &nu, &interval) || (interval && !rst_on)) continue;
        lephuff::ProgSimtScan e;
        memset(&e, 0, sizeof e);
        e.scan = (uint32_t)i; e.first_unit = (uint32_t)nunits; e.nunits = nu; e.nblocks = nb; e.rsti = interval;
        nunits += nu;
        sum_cap += (uint64_t)sv[(size_t)i].out_cap + 96;
        sv[(size_t)i].pad = lephuff::kProgScanSimt; taken[i] = interval ? 2 : 1;
        maps = maps || interval != 0;
        ps.push_back(e);
    }
    const size_t guard = 64;   // dwords
    lephuff::ProgSimtRegion r{0u, (uint32_t)ps.size(), guard * 4, 0};
    r.bytes = ((bound ? std::min<uint64_t>(sum_cap, bound + 96ull * r.nps + 4096) : sum_cap) + 15) & ~(uint64_t)15;
    if (maps) r.bytes += ((r.bytes >> 3) + 16ull * r.nps + 15) & ~(uint64_t)15;
    if (region_bytes) r.bytes = region_bytes & ~(uint64_t)15;
    const size_t unit_words = nunits * (size_t)lephuff::prog_simt_unit_words(maps);
    std::vector<uint32_t> words(unit_words + guard, 0xdeadbeefu);
    std::vector<uint32_t> scratch(guard + (size_t)r.bytes / 4 + guard, 0xa5a5a5a5u);   // (garbage: the clearing pass has to do its work)
    uint8_t* scb = reinterpret_cast<uint8_t*>(scratch.data());
    lephuff::ProgSimtUnits U;
    U.set(words.data(), nunits);
    for (auto& e : ps) for (uint32_t f = 0; f < e.nunits; f += 64) lephuff::prog_simt_units<false>(im, sv.data(), &e, &sh, U, scb, f);
    for (auto& e : ps) lephuff::prog_simt_place(sv.data(), &e, U);
    if (!ps.empty()) lephuff::prog_simt_assign(r, ps.data());
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
    for (size_t k = 0; k < guard; ++k) intact = intact && scratch[k] == 0xa5a5a5a5u && scratch[guard + (size_t)r.bytes / 4 + k] == 0xa5a5a5a5u && words[unit_words + k] == 0xdeadbeefu;
    *guards_intact = intact ? 1 : 0;
    return 0;
}

// The unit map alone: unit u of a scan of n restart units with interval rsti -> a0, a1, first restart unit and end of its interval.
extern "C" uint32_t emu_prog_rst_unit_map(uint32_t n, uint32_t rsti, int mcus, uint32_t* spans, uint32_t room) {
    lephuff::ProgUnitMap map;
    map.set(n, rsti, mcus != 0);
    const uint64_t c = map.count();
    for (uint32_t u = 0; u < c && u < room; ++u) map.span(u, spans + 4 * u, spans + 4 * u + 1, spans + 4 * u + 2, spans + 4 * u + 3);
    return (uint32_t)c;
}

// Pass 2 and what follows it on MADE-UP bit counts of a one-component DC scan (nothing else of the units is read there): the units' positions,
// the total, whether the scan was refused, and what the assign and stuff passes then answer with a region of region_bytes.
extern "C" int emu_prog_simt_rst_place_made_up(uint32_t nblocks, uint32_t rsti, const uint32_t* unit_bits, uint32_t nunits, uint32_t* positions, uint32_t* total_bits,
                                               uint32_t* refused, uint64_t region_bytes, uint32_t* buf_bytes, uint32_t* out_len) {
    static lephuff::ProgImage im;
    static lephuff::ProgScan sc;
    memset(&im, 0, sizeof im); memset(&sc, 0, sizeof sc);
    sc.cmpc = 1; sc.to = 0; sc.max_eobrun = 1; sc.rsti = (int32_t)rsti;
    im.nch[0] = (int32_t)nblocks; im.ncv[0] = 1; im.bch[0] = (int32_t)nblocks; im.bcv[0] = 1;
    uint32_t nb = 0, nu = 0, interval = 0;
    if (!lephuff::prog_simt_takes(im, sc, &nb, &nu, &interval) || nu != nunits) return 1;
    lephuff::ProgSimtScan e;
    memset(&e, 0, sizeof e);
    e.nunits = nu; e.nblocks = nb; e.rsti = interval;
    std::vector<uint32_t> words((size_t)nu * (size_t)lephuff::prog_simt_unit_words(interval != 0), 0xdeadbeefu);
    lephuff::ProgSimtUnits U;
    U.set(words.data(), nu);
    memcpy(U.bits, unit_bits, (size_t)nu * 4);
    lephuff::prog_simt_place(&sc, &e, U);
    memcpy(positions, U.bits, (size_t)nu * 4);
    *total_bits = e.total_bits; *refused = e.refused;
    lephuff::ProgSimtRegion r{0u, 1u, 0, region_bytes};
    lephuff::prog_simt_assign(r, &e);
    *buf_bytes = e.buf_bytes;
    *out_len = 0;
    if (e.buf_bytes == 0) { uint8_t none[16]; lephuff::prog_simt_stuff(&im, &sc, e, none, none, out_len); }
    return 0;
}
