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
#include "prog_simt_driver.h"

// The scans of one image as lep_gpu_huffman_progressive_encode_device routes them: lep_huffprog_simt.h's form where it takes the scan
// (one with a restart interval: where rst_on says so), the wavefront form (lep_huffprog.h) for the rest; all lane-form scans share one
// region of bit buffers.  Every pass one emulated wavefront after the other, unit arrays and region filled with garbage first
// (prog_simt_driver.h, over the launch code's own plan).
// taken[i]: 0 wavefront form, 1 lane form, 2 lane form with restart intervals.  region_bytes > 0 stands in for the launch code's region size.
// *guards_intact: the words in front of and behind the region (and behind the unit arrays) still hold what they were filled with.
extern "C" int emu_huffman_progressive_encode_lanes(const lep_huffprog_image* img, const lep_huffprog_scan* scans, int nscan, uint8_t* out, uint32_t* corr, uint32_t* out_len,
                                                    int32_t* taken, uint64_t region_bytes, int rst_on, int32_t* guards_intact) {
    return emu_prog_simt_drive(img, scans, nscan, out, corr, out_len, taken, region_bytes, rst_on != 0, nullptr, guards_intact);   // (scans of sequential frames are not this file's subject)
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

// The back end both lane writers share (lep_huff_simt.h), on made-up buffers: the stuffing loop alone ...
extern "C" uint32_t emu_simt_stuff_bytes(const uint32_t* buf, uint32_t nb, const uint32_t* marker_map, uint8_t* out, uint32_t cap) {
    return lephuff::simt_stuff_bytes(buf, nb, marker_map, out, cap);
}
// ... and the sequential writer's pass 2 on MADE-UP bit counts: MCU rows [row0, row1) of an image mcuh MCUs wide and mcuv high, the segment
// starting with overhang_bits bits of a byte.  Returns 1 when the unit map does not come to nunits units.
extern "C" int emu_simt_enc_place_made_up(int mcuh, int mcuv, int rsti, uint32_t rst_limit, int row0, int row1, uint32_t overhang_bits, const uint32_t* unit_bits, uint32_t nunits,
                                          uint32_t* positions, uint32_t* total_bits) {
    static lephuff::HuffImage im;
    lephuff::HuffSegment seg;
    memset(&im, 0, sizeof im); memset(&seg, 0, sizeof seg);
    im.mcuh = mcuh; im.mcuv = mcuv; im.mcuc = mcuh * mcuv; im.rsti = rsti; im.rst_limit = rst_limit;
    seg.mcu_row0 = row0; seg.mcu_row1 = row1; seg.overhang = overhang_bits << 8;
    lephuff::SimtUnitMap map;
    map.set(row0 * mcuh, row1 * mcuh, rsti);
    if (map.count() != nunits) return 1;
    lephuff::SimtEncSeg es;
    memset(&es, 0, sizeof es);
    es.nunits = nunits;
    std::vector<uint32_t> plain(nunits, 0xdeadbeefu);
    memcpy(positions, unit_bits, (size_t)nunits * 4);
    lephuff::simt_enc_place(&im, &seg, &es, positions, plain.data());
    *total_bits = es.total_bits;
    return 0;
}
