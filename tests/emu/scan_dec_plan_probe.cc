// scan_dec_plan_probe.cc -- TEST ONLY: the scan decoders' launch plans (lep_huffdec_simt.h simt_dec_plan, lep_scan_decode_plan.h
// prog_dec_plan) on descriptors a test made up -- only geometry, flags, scan_len, rsti, level, band and frame pointer are looked at, no
// scan byte is read.  tests/test_scan_decode_plan.py builds it as a library; with -DSCAN_DEC_PLAN_MAIN it is a program of its own that
// makes a launch of each kind and calls both plans (for a run under -fsanitize=address,undefined).  Never linked into the product.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define LEP_DEV inline
#include "../../include/lepton_mi355x.h"
#include "../../lepton_amd/csrc/lep_derive.h"
#include "../../lepton_amd/csrc/lep_scan_decode_plan.h"

static_assert(sizeof(lep_huffdec_image) == sizeof(lephuff::HuffDecImage) && sizeof(lep_huffprogdec_scan) == sizeof(lephuff::ProgDecScan), "C ABI mirrors");

// head[5] = {nw_plain, nsub_all, nslots, L, wavefronts}; per_image[nimg][5] = {first, nsub, sub_bits, changed[0], slots};
// waves[.][2] = {image, first_sub}, as many as wave_cap holds.  Returns what the plan returns.
extern "C" int emu_simt_dec_plan(const lep_huffdec_image* images, int nimg, uint32_t forced_bits, uint64_t target_lanes, uint64_t* head, uint32_t* per_image, uint32_t* waves,
                                 uint32_t wave_cap) {
    lephuff::SimtDecPlan plan;
    const int rc = lephuff::simt_dec_plan(reinterpret_cast<const lephuff::HuffDecImage*>(images), nimg, forced_bits, target_lanes, &plan);
    head[0] = (uint64_t)plan.nw_plain; head[1] = plan.nsub_all; head[2] = plan.nslots; head[3] = plan.L; head[4] = plan.waves.size();
    if (rc) return rc;
    for (int i = 0; i < nimg; ++i) {
        const lephuff::SimtImage& si = plan.si[(size_t)i];
        const uint32_t v[5] = {si.first, si.nsub, si.sub_bits, (uint32_t)si.changed[0], si.slots};
        memcpy(per_image + 5 * i, v, sizeof v);
    }
    for (size_t w = 0; w < plan.waves.size() && w < wave_cap; ++w) { waves[2 * w] = plan.waves[w].image; waves[2 * w + 1] = plan.waves[w].first_sub; }
    return 0;
}

// knobs[7] = {lanes, win, rst, piece_floor, pipeline, pipeline_max, split}.  The plan as a list of numbers, a scan named by its result_off
// (a sequential frame's by t.rows_off):
//   n, rows_off x n (a: lanes);  n, rows_off x n (a: single wave);
//   n, {order, result_off, pad} x n, ncut, cut x ncut, pipelined, any_win, ndeps, dep[4] x ndeps (b);
//   n, {result_off, pad} x n, pcut x 65, n, {result_off, pad, piece0, npieces} x n, rcut x 65, pieces, any_win (c).
// Returns how many numbers, -1 where the plan refuses the launch, -2 where cap is too small.
extern "C" int emu_prog_dec_plan(const lep_huffprogdec_scan* scans, int nscan, const int64_t* knobs, int64_t* out, int cap) {
    lephuff::ProgDecOptions o;
    o.lanes = knobs[0] != 0; o.win = knobs[1] != 0; o.rst = knobs[2] != 0; o.piece_floor = (uint32_t)knobs[3];
    o.pipeline = knobs[4] != 0; o.pipeline_max = (int)knobs[5]; o.split = knobs[6] != 0;
    lephuff::ProgDecPlan plan;
    if (lephuff::prog_dec_plan(reinterpret_cast<const lephuff::ProgDecScan*>(scans), nscan, o, &plan)) return -1;
    std::vector<int64_t> v;
    for (const auto* list : {&plan.seq_lanes, &plan.seq_single}) { v.push_back((int64_t)list->size()); for (const auto& im : *list) v.push_back((int64_t)im.rows_off); }
    const auto& b = plan.b;
    v.push_back((int64_t)b.sorted.size());
    for (size_t k = 0; k < b.sorted.size(); ++k) { v.push_back(b.order[k]); v.push_back((int64_t)b.sorted[k].result_off); v.push_back(b.sorted[k].pad); }
    v.push_back((int64_t)b.cut.size());
    for (int x : b.cut) v.push_back(x);
    v.push_back(b.pipelined); v.push_back(b.any_win);
    v.push_back((int64_t)b.deps.size());
    for (const auto& d : b.deps) for (int x : d.dep) v.push_back(x);
    const auto& c = plan.c;
    v.push_back((int64_t)c.plain.size());
    for (const auto& sc : c.plain) { v.push_back((int64_t)sc.result_off); v.push_back(sc.pad); }
    for (int x : c.pcut) v.push_back(x);
    v.push_back((int64_t)c.rst.size());
    for (size_t k = 0; k < c.rst.size(); ++k) { v.push_back((int64_t)c.rst[k].result_off); v.push_back(c.rst[k].pad); v.push_back(c.plans[k].piece0); v.push_back(c.plans[k].npieces); }
    for (int x : c.rcut) v.push_back(x);
    v.push_back(c.pieces); v.push_back(c.any_win);
    if ((int)v.size() > cap) return -2;
    memcpy(out, v.data(), v.size() * sizeof(int64_t));
    return (int)v.size();
}

#ifdef SCAN_DEC_PLAN_MAIN
// the launches of tests/test_scan_decode_plan.py, made here: five images for the lane decoder (wide blind, plain, interval, wide blind,
// plain), the scans of three files interleaved for the progressive decoder, every knob in turn, and the launches both plans refuse
static lep_huffdec_image image(uint32_t scan_len, int hs0, int same_tables, int mcuc, int rsti, int flags) {
    lep_huffdec_image im;
    memset(&im, 0, sizeof im);
    im.scan_len = scan_len; im.ncomp = 3; im.mcuh = mcuc; im.mcuv = 1; im.mcuc = mcuc; im.rsti = rsti; im.flags = flags;
    for (int c = 0; c < 3; ++c) { im.hs[c] = im.vs[c] = c ? 1 : hs0; im.scan_cmp[c] = c; im.dc_tbl[c] = im.ac_tbl[c] = (c && !same_tables) ? 1 : 0; }
    return im;
}
static lep_huffprogdec_scan scan(uintptr_t frame, int id, int level, int from, int to, int sah, int cmpc, int rsti, int flags, uint32_t scan_len) {
    lep_huffprogdec_scan s;
    memset(&s, 0, sizeof s);
    s.t = image(scan_len, 2, 0, 100, rsti, flags);
    s.t.blocks[0] = reinterpret_cast<int16_t*>(frame);
    s.t.rows_off = (uint64_t)id; s.result_off = (uint64_t)id;
    s.cmpc = cmpc; s.from = from; s.to = to; s.sah = sah; s.level = level;
    for (int c = 0; c < 4; ++c) { s.cmp[c] = c < cmpc ? c : 0; s.nch[c] = 20; s.ncv[c] = 10; s.bcv[c] = 10; }
    return s;
}
int main() {
    const lep_huffdec_image five[5] = {image(20000, 2, 1, 50, 0, 0), image(1000, 1, 0, 50, 0, 0), image(3000, 2, 0, 103, 5, LEP_HUFFDEC_RST_TABLE), image(9000, 2, 1, 50, 0, 0), image(12800, 1, 0, 50, 0, 0)};
    uint64_t head[5];
    uint32_t per[25], waves[64];
    if (emu_simt_dec_plan(five, 5, 1000, 64 * 8192 * 2, head, per, waves, 32) || head[0] != 4 || head[1] != 357 || head[2] != 228 || head[3] != 1024 || head[4] != 9) return 1;
    if (emu_simt_dec_plan(five, 5, 0, 1000, head, per, waves, 32) || head[3] != 8192) return 2;
    const lep_huffdec_image refused[3] = {image(1000, 2, 0, 50, 5, 0), image(1000, 2, 0, 0x7fffffff, 1, LEP_HUFFDEC_RST_TABLE), image(1000, 2, 0, 0x7fffffff, 1, LEP_HUFFDEC_RST_TABLE)};
    if (!emu_simt_dec_plan(refused, 1, 0, 1000, head, per, waves, 32) || !emu_simt_dec_plan(refused + 1, 2, 0, 1000, head, per, waves, 32)) return 3;
    const uintptr_t A = 0x1000, B = 0x2000, Cf = 0x3000;
    const int T = LEP_HUFFDEC_RST_TABLE;
    std::vector<lep_huffprogdec_scan> s = {scan(A, 0, 0, 0, 0, 0, 3, 2, T, 10000), scan(B, 1, 0, 0, 0, 0, 3, 0, 0, 500),  scan(Cf, 2, 0, 0, 63, 0, 1, 3, 0, 700), scan(A, 3, 1, 1, 5, 0, 1, 2, T, 4000),
                                           scan(B, 4, 1, 1, 5, 0, 1, 0, 0, 500),    scan(Cf, 5, 0, 0, 63, 0, 2, 0, 0, 700), scan(A, 6, 1, 6, 63, 0, 1, 0, 0, 900),  scan(B, 7, 2, 1, 5, 1, 1, 0, 0, 500),
                                           scan(A, 8, 0, 1, 5, 0, 1, 4, 0, 900),    scan(B, 9, 1, 0, 0, 1, 3, 0, 0, 500)};
    s[8].cmp[0] = 1;
    std::vector<int64_t> out(1024);
    for (int knob = -1; knob < 7; ++knob) {
        int64_t knobs[7] = {1, 1, 1, 1024, 1, 16384, 0};
        if (knob >= 0) knobs[knob] = knob == 6 ? 1 : (knob == 5 ? 3 : (knob == 3 ? 1 : 0));
        const int n = emu_prog_dec_plan(s.data(), (int)s.size(), knobs, out.data(), (int)out.size());
        if (n <= 0) return 4;
        printf("knob %d: %d numbers\n", knob, n);
    }
    const int64_t on[7] = {1, 1, 1, 1024, 1, 16384, 0};
    s[7].level = 64;
    if (emu_prog_dec_plan(s.data(), (int)s.size(), on, out.data(), (int)out.size()) != -1) return 5;
    s[7].level = 2; s[2].cmpc = 0;
    if (emu_prog_dec_plan(s.data(), (int)s.size(), on, out.data(), (int)out.size()) != -1) return 6;
    std::vector<lep_huffprogdec_scan> many;          // seventeen scans of 126,322,568 pieces each: more than an int32 counts
    for (int i = 0; i < 20; ++i) { many.push_back(scan(A, i, 0, 0, 0, 0, 3, 1, T, (1u << 27) - 16)); many.back().t.mcuc = 0x7fffffff; }
    const int64_t floor1[7] = {1, 1, 1, 1, 1, 16384, 0};
    if (emu_prog_dec_plan(many.data(), (int)many.size(), floor1, out.data(), (int)out.size()) != -1) return 7;
    puts("scan decode plans: ok");
    return 0;
}
#endif
