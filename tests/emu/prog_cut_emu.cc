// prog_cut_emu.cc -- TEST ONLY: the scan kernels over progressive files cut inside a scan (prog_cut_driver.h), compiled with g++ as a
// lane-loop emulation (lep_wave.h).  Never linked into the product.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
#define LEP_DEV inline
#include "../../lepton_amd/csrc/lep_derive.h"
#include "prog_cut_driver.h"

extern "C" int emu_prog_cut_decode_file(const lep_huffprogdec_scan* scans, int nscan, const uint8_t* raw, size_t raw_len, int win, int pipelined, int misalign,
                                        lep_huffdec_row* rows, int32_t* win_taken, int32_t* declined) {
    return emu_prog_cut_decode(reinterpret_cast<const lephuff::ProgDecScan*>(scans), nscan, raw, raw_len, win != 0, pipelined != 0, misalign != 0,
                               reinterpret_cast<lephuff::HuffDecRow*>(rows), win_taken, declined);
}

extern "C" int emu_prog_cut_write_file(const lep_huffprog_image* img, const lep_huffprog_scan* scans, int nscan, int nsegs, const int32_t* coded_blocks, uint8_t* out,
                                       uint32_t* corr, uint32_t* out_len, int32_t* taken, int32_t* guards_intact) {
    return emu_prog_cut_write(img, scans, nscan, nsegs, coded_blocks, out, corr, out_len, taken, guards_intact);
}
