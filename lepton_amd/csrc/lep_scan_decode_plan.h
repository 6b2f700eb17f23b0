// lep_scan_decode_plan.h -- the launch plan of the progressive scan decoder (lep_gpu_huffman_progressive_decode_device): which of a
// launch's scans go to which kernels, in which order and with which marks, descriptors and dependencies.  Host code only; the launch code
// (lep_gpu.hip) lays out, uploads and launches what the plan says and decides nothing, and tests/emu steps the same plan on the CPU
// (tests/emu/scan_dec_driver.h).  The lane decoder of sequential scans has its own beside its passes: lep_huffdec_simt.h simt_dec_plan.
#pragma once
#include "lep_huffdec_simt.h"
#include "lep_huffprogdec_rst.h"

namespace lephuff {

struct ProgDecOptions {             // the launch object's knobs (lep_gpu.hip: LEP_HUFFDEC_SIMT, LEP_HUFFPROGDEC_WIN / _RST / _RST_FLOOR, LEP_HUFFPROG_PIPELINE / _SPLIT)
    bool lanes = true;              // scans of sequential frames: the lane decoder where it takes them (simt_dec_takes)
    bool win = true;                // the window of speculative codes (lep_huffprogdec_win.h) where it takes a scan
    bool rst = true;                // the interval form (lep_huffprogdec_rst.h) where it takes a scan
    uint32_t piece_floor = kRstPieceFloor;
    bool pipeline = true;           // small launches: all levels as one launch in which a scan follows the scans in front of it row by row
    int pipeline_max = 0;           // ... of at most this many scans: beyond what is resident at once the chip is full either way
    bool split = false;             // a measurement aid: inside a level a launch per KIND of scan
};

struct ProgDecPlan {
    // a. Scans of SEQUENTIAL frames coded in several scans (lep_huffprogdec.h sequential_scan_image): no scan depends on another, each is
    // an image of its own to the sequential kernels -- one lane per subsequence, or the single-wave kernel
    std::vector<HuffDecImage> seq_lanes, seq_single;
    // b. The scans of files WITHOUT a scan of the interval form, ordered by dependency level (stable), ProgDecScan::pad saying which
    // form decodes each.  order[k]: the scan's index in the caller's array.  cut: launch boundaries for level after level (split: level and
    // kind).  pipelined: one launch for all, with deps[k] = the scans (indices into `sorted`) that scan k follows.
    struct Levels {
        std::vector<ProgDecScan> sorted;
        std::vector<int> order, cut;
        std::vector<ProgDeps> deps;
        bool pipelined = false, any_win = false;
    } b;
    // c. The scans of files WITH one (the caller has put the marker positions behind their slots): such a file goes level by level as a
    // whole, every level many wavefronts per scan of that form -- none of its scans waits on a progress word.  plain / rst: the two kinds,
    // each by level, [pcut[lv], pcut[lv + 1]) and [rcut[lv], rcut[lv + 1]) being level lv's; plans[k]: the pieces of rst[k], piece0
    // counting through the launch (level lv's pieces: piece_cut(lv) .. piece_cut(lv + 1)).
    struct Pieces {
        std::vector<ProgDecScan> plain, rst;
        std::vector<ProgRstScan> plans;
        std::vector<int> pcut, rcut;
        uint32_t pieces = 0;
        bool any_win = false;
        uint32_t piece_cut(int lv) const { return rcut[(size_t)lv] < (int)plans.size() ? plans[(size_t)rcut[(size_t)lv]].piece0 : pieces; }
    } c;
    // d. Scans of files that END INSIDE them (kHuffDecEarlyEof in t.flags; a file's last scan) which the window form does not take -- a
    // restart interval, a slot that is not aligned, the form switched off: only lep_huffprogdec_win.h knows the cut, so such a scan goes
    // to NO kernel.  Their result_off: the launch code marks the final record there as not written, and the file goes to the host parser.
    std::vector<uint64_t> declined;
};
// what the launch code (and the emulation) fills a declined scan's final record with, byte for byte: aux < 0, a status
constexpr int kProgDecDeclinedFill = 0x80;

// Non-zero: a sequential scan of no or more than four components, a dependency level outside 0 .. 63, more pieces than an int32 counts.
inline int prog_dec_plan(const ProgDecScan* scans, int nscan, const ProgDecOptions& o, ProgDecPlan* out) {
    *out = ProgDecPlan();
    std::vector<int> prog;          // the progressive scans, by their index in the caller's array
    for (int i = 0; i < nscan; ++i) {
        const ProgDecScan& sc = scans[i];
        if (!progdec_is_sequential(sc)) {
            if (sc.level < 0 || sc.level > 63) return 1;
            if ((sc.t.flags & kHuffDecEarlyEof) && !(o.win && prog_win_takes(sc))) { out->declined.push_back(sc.result_off); continue; }
            prog.push_back(i);
            continue;
        }
        if (sc.cmpc < 1 || sc.cmpc > 4) return 1;
        const HuffDecImage im = sequential_scan_image(sc);
        ((o.lanes && sequential_scan_for_lanes(im)) ? out->seq_lanes : out->seq_single).push_back(im);
    }
    // files with a scan of the interval form, by their frame
    std::vector<const void*> frames;
    if (o.rst)
        for (int i : prog) if (prog_rst_takes(scans[i])) frames.push_back((const void*)scans[i].t.blocks[0]);
    std::sort(frames.begin(), frames.end());
    auto marked = [&](ProgDecScan sc, bool* any_win) {
        const bool w = o.win && prog_win_takes(sc);
        sc.pad = w ? kProgDecWin : 0;
        *any_win = *any_win || w;
        return sc;
    };
    // (split: inside a level the scans of one KIND -- DC / AC, first stage / refinement, component, band -- stand together and get a launch
    // of their own, so that a kernel trace shows what each kind of scan takes)
    auto kind = [](const ProgDecScan& s) { return (s.to == 0 ? 0 : 1) * 100000 + (s.sah ? 1 : 0) * 10000 + (s.cmpc > 1 ? 9 : s.cmp[0]) * 1000 + s.from * 10 + (s.to > 9 ? 9 : s.to); };
    ProgDecPlan::Levels& b = out->b;
    ProgDecPlan::Pieces& c = out->c;
    int maxlevel = 0;
    for (int lv = 0; lv < 64; ++lv) {
        c.pcut.push_back((int)c.plain.size()); c.rcut.push_back((int)c.rst.size());
        std::vector<int> idx;       // level lv of part b
        for (int i : prog) {
            const ProgDecScan& sc = scans[i];
            if (sc.level != lv) continue;
            if (!std::binary_search(frames.begin(), frames.end(), (const void*)sc.t.blocks[0])) { idx.push_back(i); maxlevel = lv; continue; }
            if (!prog_rst_takes(sc)) { c.plain.push_back(marked(sc, &c.any_win)); continue; }
            const ProgRstScan pl = prog_rst_plan(sc, o.piece_floor, c.pieces);
            if (pl.npieces > 0x7fffffffu - c.pieces) return 1;
            c.pieces += pl.npieces;
            c.rst.push_back(sc); c.rst.back().pad = kProgDecRst;
            c.plans.push_back(pl);
        }
        if (o.split) std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return kind(scans[x]) < kind(scans[y]); });
        for (size_t q = 0; q < idx.size(); ++q) {
            if (q == 0 || (o.split && kind(scans[idx[q]]) != kind(scans[idx[q - 1]]))) b.cut.push_back((int)b.sorted.size());
            b.sorted.push_back(marked(scans[idx[q]], &b.any_win)); b.order.push_back(idx[q]);
        }
    }
    c.pcut.push_back((int)c.plain.size()); c.rcut.push_back((int)c.rst.size());
    b.cut.push_back((int)b.sorted.size());
    // Small launches wait for the chain of a file's dependent scans, not for throughput: they go out as ONE launch (prog_scan_deps
    // says no where a scan follows more than four others)
    const int nb = (int)b.sorted.size();
    b.pipelined = o.pipeline && maxlevel > 0 && nb <= o.pipeline_max;
    if (b.pipelined) {
        b.deps.resize((size_t)nb);
        b.pipelined = prog_scan_deps(b.sorted.data(), b.order.data(), nb, b.deps.data());
        if (!b.pipelined) b.deps.clear();
    }
    return 0;
}

}  // namespace lephuff
