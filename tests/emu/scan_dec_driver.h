// scan_dec_driver.h -- TEST ONLY: the scan decoders as lep_gpu_huffman_decode_simt_device and lep_gpu_huffman_progressive_decode_device
// run them, every pass one emulated wavefront after the other.  What goes where -- subsequences, wave lists, slot offsets, levels, forms,
// pieces, dependencies -- comes from simt_dec_plan (lep_huffdec_simt.h) and prog_dec_plan (lep_scan_decode_plan.h): the launch code's own
// plans.  Included by core_emu.cc and prog_rst_emu.cc, which the tests build as separate libraries.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../lepton_amd/csrc/lep_scan_decode_plan.h"

// One launch of the lane decoder.  forced_bits / the rule as the launch code's (0: the rule, for 64 * 8192 * 2 lanes).  side_array = false:
// a caller that passes none (a wide blind image is then not taken for blind).  plan_out: what the passes left in the plan's SimtImages.
inline int emu_simt_dec_drive(const lephuff::HuffDecImage* images, int nimg, uint32_t forced_bits, bool side_array, lephuff::HuffDecRow* rows, lephuff::SimtDecPlan* plan_out = nullptr) {
    static lephuff::SimtShared sh;
    static lephuff::SimtColumns cols;
    static lephuff::SimtTile tile;
    lephuff::SimtDecPlan plan;
    if (lephuff::simt_dec_plan(images, nimg, forced_bits, (uint64_t)64 * 8192 * 2, &plan)) return -1;
    std::vector<lephuff::SimtSub> buf[2] = {std::vector<lephuff::SimtSub>(plan.nsub_all), std::vector<lephuff::SimtSub>(plan.nsub_all)};
    std::vector<lephuff::SimtPlace> place(plan.nsub_all);
    // (an entry per subsequence of a wide blind image, none for any other -- but the pointer is passed all the same, as the launch code does)
    std::vector<lephuff::SimtSlots> side(plan.nslots + 1);
    lephuff::SimtSlots* slots = side_array ? side.data() : nullptr;
    const int nw = (int)plan.waves.size();
    for (int k = 0; k <= lephuff::kSimtSettle; ++k)
        for (int w = 0; w < nw; ++w) {                      // (the plain wavefronts' launch has no columns: dynamic LDS of the wide ones' only)
            const lephuff::SimtWave& wv = plan.waves[(size_t)w];
            lephuff::SimtImage* si = &plan.si[wv.image];
            lephuff::simt_guess_or_settle(images + wv.image, &sh, si, buf[(k + 1) & 1].data() + si->first, buf[k & 1].data() + si->first, wv.first_sub, k, slots,
                                          w < plan.nw_plain ? nullptr : &cols);
        }
    const lephuff::SimtSub* fin = buf[lephuff::kSimtSettle & 1].data();
    for (int i = 0; i < nimg; ++i) lephuff::simt_place(images + i, &plan.si[(size_t)i], fin + plan.si[(size_t)i].first, place.data() + plan.si[(size_t)i].first, lephuff::kSimtSettle, rows, slots);
    for (const lephuff::SimtWave& wv : plan.waves) {
        lephuff::SimtImage* si = &plan.si[wv.image];
        lephuff::simt_write(images + wv.image, &sh, &tile, si, fin + si->first, place.data() + si->first, rows, wv.first_sub);
    }
    for (int i = 0; i < nimg; ++i) lephuff::simt_finish(images + i, &plan.si[(size_t)i], rows);
    if (plan_out) *plan_out = plan;
    return 0;
}

// One launch of the progressive decoder.  deps_out[nscan][4] (optional): the scans each scan follows in a pipelined launch, indices into
// the caller's array, -1 = none -- all -1 where the plan does not pipeline.  win_taken / rst_taken[nscan] / pieces (optional): how many
// scans the window form decoded, which scans the interval form, in how many pieces.
// Returns -1: the plan refuses the launch; -3: a scan follows one behind it in the launch; -4: a pipelined scan did not say it was done.
inline int emu_prog_dec_drive(const lephuff::ProgDecScan* scans, int nscan, const lephuff::ProgDecOptions& o, lephuff::HuffDecRow* rows, int32_t* deps_out = nullptr,
                              int32_t* win_taken = nullptr, int32_t* rst_taken = nullptr, uint32_t* pieces = nullptr) {
    static lephuff::HuffDecShared sh;
    static lephuff::ProgWinShared ws;
    lephuff::ProgDecPlan plan;
    if (lephuff::prog_dec_plan(scans, nscan, o, &plan)) return -1;
    if (deps_out) for (int i = 0; i < 4 * nscan; ++i) deps_out[i] = -1;
    // a. sequential frames' scans
    if (!plan.seq_lanes.empty()) { if (int rc = emu_simt_dec_drive(plan.seq_lanes.data(), (int)plan.seq_lanes.size(), 0, true, rows)) return rc; }
    for (const lephuff::HuffDecImage& im : plan.seq_single) { lephuff::HuffDecWave w; w.run(&im, &sh, rows); }
    // (lep_huffprogdec_win_kernel / _win_pipelined_kernel: the mark says which form)
    auto run_scan = [&](const lephuff::ProgDecScan* sc) {
        if (sc->pad & lephuff::kProgDecWin) { lephuff::ProgWinWave w; w.run_scan_win<false>(sc, &ws, rows); }
        else { lephuff::ProgDecWave w; w.run_scan<false>(sc, &sh, rows); }
    };
    int nwin = 0;
    // b. files without a scan of the interval form: the one pipelined launch in launch order, or launch after launch
    const lephuff::ProgDecPlan::Levels& b = plan.b;
    const int nb = (int)b.sorted.size();
    for (const lephuff::ProgDecScan& sc : b.sorted) nwin += (sc.pad & lephuff::kProgDecWin) != 0;
    if (b.pipelined) {
        std::vector<uint32_t> progress((size_t)nb, 0u);
        for (int k = 0; k < nb; ++k) {
            for (int d = 0; d < 4; ++d) {
                const int j = b.deps[(size_t)k].dep[d];
                if (j >= k) return -3;
                if (deps_out && j >= 0) deps_out[b.order[(size_t)k] * 4 + d] = b.order[(size_t)j];
            }
            const lephuff::ProgDecScan* sc = &b.sorted[(size_t)k];
            if (sc->pad & lephuff::kProgDecWin) { lephuff::ProgWinWave w; w.run_scan_win<true>(sc, &ws, rows, &b.deps[(size_t)k], progress.data(), k); }
            else { lephuff::ProgDecWave w; w.run_scan<true>(sc, &sh, rows, &b.deps[(size_t)k], progress.data(), k); }
            if (progress[(size_t)k] != 0x7fffffffu) return -4;      // every scan says when it is done, whatever happened to it
        }
    } else
        for (size_t q = 0; q + 1 < b.cut.size(); ++q)
            for (int k = b.cut[q]; k < b.cut[q + 1]; ++k) run_scan(&b.sorted[(size_t)k]);
    // c. files with one: level after level, the pieces of the launch as lep_huffprogdec_rst_kernel finds their scans; then the reduce step
    const lephuff::ProgDecPlan::Pieces& c = plan.c;
    for (const lephuff::ProgDecScan& sc : c.plain) nwin += (sc.pad & lephuff::kProgDecWin) != 0;
    std::vector<lephuff::ProgRstOut> outs(c.pieces);
    if (!outs.empty()) memset(outs.data(), 0xee, outs.size() * sizeof outs[0]);
    for (int lv = 0; lv < 64; ++lv) {
        for (int k = c.pcut[(size_t)lv]; k < c.pcut[(size_t)lv + 1]; ++k) run_scan(&c.plain[(size_t)k]);
        int at = c.rcut[(size_t)lv];
        for (uint32_t piece = c.piece_cut(lv); piece < c.piece_cut(lv + 1); ++piece) {
            while (at + 1 < c.rcut[(size_t)lv + 1] && c.plans[(size_t)at + 1].piece0 <= piece) ++at;
            const lephuff::ProgRstScan& pl = c.plans[(size_t)at];
            const uint32_t first = (piece - pl.piece0) * pl.ipp;
            if (piece - pl.piece0 >= pl.npieces || first >= pl.nint) continue;
            lephuff::ProgRstWave w;
            w.run_piece(&c.rst[(size_t)at], &ws, rows, pl.nint, first, pl.nint - first < pl.ipp ? pl.nint - first : pl.ipp, &outs[piece]);
        }
    }
    for (size_t k = 0; k < c.rst.size(); ++k) lephuff::prog_rst_reduce(&c.rst[k], &c.plans[k], outs.data(), rows);
    if (win_taken) *win_taken = nwin;
    if (pieces) *pieces = c.pieces;
    if (rst_taken)
        for (int i = 0; i < nscan; ++i) {                   // (a scan is known by where its final record goes)
            rst_taken[i] = 0;
            for (const lephuff::ProgDecScan& sc : c.rst) rst_taken[i] |= sc.result_off == scans[i].result_off && sc.t.blocks[0] == scans[i].t.blocks[0];
        }
    return 0;
}
