// prog_cut_plan_probe.cc -- TEST ONLY: where prog_dec_plan (lep_scan_decode_plan.h) sends every scan of a launch, as numbers: the scans of
// part b, the plain and the interval scans of part c, the sequential frames' scans and the scans it sends to NO kernel (a scan flagged
// LEP_HUFFDEC_EARLY_EOF that the window form does not take).  No scan byte is read.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
#define LEP_DEV inline
#include "../../lepton_amd/csrc/lep_derive.h"
#include "../../lepton_amd/csrc/lep_scan_decode_plan.h"

// out: count, then (result_off, pad) per scan, for b / c.plain / c.rst; count, result_off per declined scan; count of sequential scans.
// Returns the numbers written, -1: the plan refuses the launch, -2: cap.
extern "C" int emu_prog_cut_plan(const lep_huffprogdec_scan* scans, int nscan, int win, int rst, int pipeline, int64_t* out, int cap) {
    lephuff::ProgDecOptions o;
    o.lanes = true; o.win = win != 0; o.rst = rst != 0; o.pipeline = pipeline != 0; o.pipeline_max = 1 << 20;
    lephuff::ProgDecPlan plan;
    if (lephuff::prog_dec_plan(reinterpret_cast<const lephuff::ProgDecScan*>(scans), nscan, o, &plan)) return -1;
    std::vector<int64_t> v;
    auto list = [&](const std::vector<lephuff::ProgDecScan>& s) {
        v.push_back((int64_t)s.size());
        for (const lephuff::ProgDecScan& sc : s) { v.push_back((int64_t)sc.result_off); v.push_back(sc.pad); }
    };
    list(plan.b.sorted); list(plan.c.plain); list(plan.c.rst);
    v.push_back((int64_t)plan.declined.size());
    for (uint64_t r : plan.declined) v.push_back((int64_t)r);
    v.push_back((int64_t)(plan.seq_lanes.size() + plan.seq_single.size()));
    v.push_back(plan.b.pipelined ? 1 : 0);
    for (const lephuff::ProgDeps& d : plan.b.deps) for (int i = 0; i < 4; ++i) v.push_back(d.dep[i]);
    if ((int)v.size() > cap) return -2;
    memcpy(out, v.data(), v.size() * sizeof(int64_t));
    return (int)v.size();
}
