// prog_rst_emu.cc -- TEST ONLY: lep_huffprogdec_rst.h (progressive scans with restart intervals, one wavefront per piece of consecutive
// intervals) compiled with g++ as a lane-loop emulation (lep_wave.h), with the launch code's routing around it.  Never linked into the product.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
#define LEP_DEV inline
#include "../../lepton_amd/csrc/lep_derive.h"
#include "../../lepton_amd/csrc/lep_huffprogdec_rst.h"

// The scans of one file, level by level as the launch code runs a file that has a scan of this form: scans flagged
// LEP_HUFFDEC_RST_TABLE (the caller has put the marker positions behind the slot) piece by piece and then the reduce step, the window
// form where it takes the scan, lep_huffprogdec.h for the rest; scans of sequential frames go to the single-wave sequential kernel.
static void run_levels(const lep_huffprogdec_scan* scans, int nscan, lephuff::HuffDecRow* rows, bool rst, uint32_t piece_floor, int32_t* taken, uint32_t* pieces) {
    static lephuff::HuffDecShared sh;
    static lephuff::ProgWinShared ws;
    for (int lv = 0; lv < 64; ++lv)
        for (int i = 0; i < nscan; ++i) {
            const lephuff::ProgDecScan& sc = *reinterpret_cast<const lephuff::ProgDecScan*>(scans + i);
            if (sc.level != lv) continue;
            if (lephuff::progdec_is_sequential(sc)) {
                const lephuff::HuffDecImage im = lephuff::sequential_scan_image(sc);
                lephuff::HuffDecImage one = im;
                one.rows_off = 0;
                lephuff::HuffDecWave w;
                w.run(&one, &sh, rows + im.rows_off);
            } else if (rst && lephuff::prog_rst_takes(sc)) {
                const lephuff::ProgRstScan plan = lephuff::prog_rst_plan(sc, piece_floor ? piece_floor : lephuff::kRstPieceFloor, 0);
                std::vector<lephuff::ProgRstOut> outs(plan.npieces);
                memset(outs.data(), 0xee, outs.size() * sizeof outs[0]);
                for (uint32_t p = 0; p < plan.npieces; ++p) {
                    const uint32_t first = p * plan.ipp, count = plan.nint - first < plan.ipp ? plan.nint - first : plan.ipp;
                    lephuff::ProgRstWave w;
                    w.run_piece(&sc, &ws, rows, plan.nint, first, count, &outs[p]);
                }
                lephuff::prog_rst_reduce(&sc, &plan, outs.data(), rows);
                taken[i] = 1;
                *pieces += plan.npieces;
            } else if (lephuff::prog_win_takes(sc)) {
                lephuff::ProgWinWave w;
                w.run_scan_win<false>(&sc, &ws, rows);
            } else {
                lephuff::ProgDecWave w;
                w.run_scan<false>(&sc, &sh, rows);
            }
        }
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
    for (int i = 0; i < nscan; ++i) taken[i] = 0;
    run_levels(scans, nscan, rows, true, piece_floor, taken, &pieces);
    bool again = false;
    for (int i = 0; i < nscan; ++i) again = again || (taken[i] && (rows[scans[i].result_off].aux >> 8) != 0);
    if (again) {
        for (int c = 0; c < scans[0].t.ncomp && c < 4; ++c) memset(scans[0].t.blocks[c], 0, (size_t)scans[0].t.bch[c] * (size_t)scans[0].bcv[c] * 128);
        int32_t none[64] = {0};
        uint32_t zero = 0;
        run_levels(scans, nscan, rows, false, 0, none, &zero);
    }
    if (pieces_out) *pieces_out = pieces;
    if (second_chance) *second_chance = again ? 1 : 0;
    return 0;
}
