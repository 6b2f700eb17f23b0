// prog_rst_emu.cc -- TEST ONLY: lep_huffprogdec_rst.h (progressive scans with restart intervals, one wavefront per piece of consecutive
// intervals) compiled with g++ as a lane-loop emulation (lep_wave.h), with the launch code's routing around it.  Never linked into the product.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
#define LEP_DEV inline
#include "../../lepton_amd/csrc/lep_derive.h"
#include "scan_dec_driver.h"

// The scans of one file as the launch code runs them (scan_dec_driver.h over lep_scan_decode_plan.h's plan): a file that has a scan flagged
// LEP_HUFFDEC_RST_TABLE (the caller has put the marker positions behind the slot) level by level -- those scans piece by piece and then the
// reduce step, the window form where it takes the scan, lep_huffprogdec.h for the rest; scans of sequential frames go to the single-wave
// sequential kernel.  rst = false: the interval form off, whatever the descriptors carry.
static int run_levels(const lep_huffprogdec_scan* scans, int nscan, lephuff::HuffDecRow* rows, bool rst, uint32_t piece_floor, int32_t* taken, uint32_t* pieces) {
    lephuff::ProgDecOptions o;
    o.lanes = false; o.win = true; o.rst = rst; o.pipeline = false; o.split = false;
    o.piece_floor = piece_floor ? piece_floor : lephuff::kRstPieceFloor;
    return emu_prog_dec_drive(reinterpret_cast<const lephuff::ProgDecScan*>(scans), nscan, o, rows, nullptr, nullptr, taken, pieces);
}

// piece_floor: bytes of scan per piece (0: the product's; 1: a piece per interval; 0xffffffff: the whole scan in one piece).
// taken[i] = 1 where scan i went through the new form; pieces_out: pieces in all.
// *second_chance = 1: a scan of the new form ended with a status -- an interval of a damaged file that does not end at its marker is
// something the reference, which never looks at where the markers stood, may still decode -- and the file went through the older forms
// again, its frame wiped first, as the batch pipeline does (lep_batch.hip): the host parser is asked for exactly the files it was asked for before.
extern "C" int emu_huffman_progressive_decode_rst(const lep_huffprogdec_scan* scans, int nscan, lep_huffdec_row* rows_, uint32_t piece_floor, int32_t* taken, uint32_t* pieces_out,
                                                  int32_t* second_chance) {
    lephuff::HuffDecRow* rows = reinterpret_cast<lephuff::HuffDecRow*>(rows_);
    uint32_t pieces = 0;
    if (int rc = run_levels(scans, nscan, rows, true, piece_floor, taken, &pieces)) return rc;
    bool again = false;
    for (int i = 0; i < nscan; ++i) again = again || (taken[i] && (rows[scans[i].result_off].aux >> 8) != 0);
    if (again) {
        for (int c = 0; c < scans[0].t.ncomp && c < 4; ++c) memset(scans[0].t.blocks[c], 0, (size_t)scans[0].t.bch[c] * (size_t)scans[0].bcv[c] * 128);
        if (int rc = run_levels(scans, nscan, rows, false, 0, nullptr, nullptr)) return rc;
    }
    if (pieces_out) *pieces_out = pieces;
    if (second_chance) *second_chance = again ? 1 : 0;
    return 0;
}
