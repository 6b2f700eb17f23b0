// core_emu.cc -- TEST ONLY: compiles the kernel headers under lepton_amd/csrc with g++ as lane-loop emulations (lep_wave.h) -- and the
// single-lane coder of round 1 (lep_core_coder.h) -- so that kernel logic can be single-stepped and diffed against the oracle
// without a GPU.  Never linked into the product.
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>
#define LEP_DEV inline
#include "../../lepton_amd/csrc/lep_derive.h"
#include "lep_core_coder.h"   // the single-lane coder of round 1: test infrastructure

using namespace lepdev;

template <bool DEC>
static int run(const lep_image_desc* d, int y0, int y1, int is_last, uint8_t* stream, uint32_t* len, uint32_t cap, uint32_t* bins) {
    ImageDev img;
    int rc = derive_image(*d, &img, !DEC);
    if (rc) return rc;
    std::vector<uint32_t> model(kModelBranches, kBranchInit);
    std::vector<NSum> ns(img.ns_total);
    memset(ns.data(), 0, ns.size() * sizeof(NSum));
    SegDev seg;
    seg.image = 0; seg.y0 = y0; seg.y1 = y1; seg.is_last = is_last; seg.stream_off = 0; seg.stream_cap = cap;
    SegmentCoder<DEC> sc;
    if constexpr (DEC) sc.bc.init_stream(stream, *len); else sc.bc.init_stream(stream, cap);
    rc = sc.run(&img, seg, model.data(), ns.data());
    if constexpr (!DEC) { *len = sc.bc.finish(); if (sc.bc.overflow) rc = LEP_BUFFER_TOO_SMALL; }
    if (bins) *bins = sc.nbins;
    return rc;
}

extern "C" int emu_encode_segment(const lep_image_desc* d, int y0, int y1, int is_last, uint8_t* out, uint32_t cap, uint32_t* len, uint32_t* bins) {
    return run<false>(d, y0, y1, is_last, out, len, cap, bins);
}
extern "C" int emu_decode_segment(const lep_image_desc* d, int y0, int y1, int is_last, const uint8_t* in, uint32_t len, uint32_t* bins) {
    return run<true>(d, y0, y1, is_last, const_cast<uint8_t*>(in), &len, 0, bins);
}


// The v3 / v4 decoders read the stream as ALIGNED dwords (the dword that holds the first and the one that holds the last byte
// are loaded whole, the bytes outside the stream masked off) -- on the device every stream sits in an arena that is padded to
// 256 bytes.  Give the emulation the same guarantee (and keep the caller's alignment phase), so that an address sanitizer
// run of these tests only reports real out-of-bounds accesses.
struct PaddedStream {
    std::vector<uint8_t> arena;
    const uint8_t* p;
    PaddedStream(const uint8_t* in, uint32_t len) : arena((size_t)len + 24, 0) {
        uint8_t* base = arena.data() + 8;
        base -= (uintptr_t)base & 3;                 // 4-byte aligned, at least 4 bytes into the arena
        uint8_t* q = base + ((uintptr_t)in & 3);     // same phase as the caller's pointer
        if (len) memcpy(q, in, len);
        p = q;
    }
};

// v3 encoder (lep_enc3.h) as a 64-lane loop emulation
#include "../../lepton_amd/csrc/lep_enc3.h"
extern "C" int emu_encode_segment_v3(const lep_image_desc* d, int y0, int y1, int is_last, uint8_t* out, uint32_t cap, uint32_t* len, uint32_t* bins) {
    ImageDev img;
    int rc = derive_image(*d, &img, true);
    if (rc) return rc;
    std::vector<uint32_t> model(kModelBranches, kBranchInit);
    std::vector<NSum> ns(img.ns_total);
    memset(ns.data(), 0, ns.size() * sizeof(NSum));
    SegDev seg;
    seg.image = 0; seg.y0 = y0; seg.y1 = y1; seg.is_last = is_last; seg.stream_off = 0; seg.stream_cap = cap;
    static lep3::Enc3Shared sh;
    static lep3::Enc3Pipe pipe;   // LEP_EMU_ENC_PIPE=1: the producer half of the two-wave kernel; its hand-over runs the consumer's step in place
    lep3::Enc3Wave w;
    rc = w.run(&img, seg, model.data(), ns.data(), &sh, out, cap, getenv("LEP_EMU_ENC_PIPE") ? &pipe : nullptr);
    if (rc) return rc;
    *len = w.bc.finish();
    if (w.bc.overflow) return LEP_BUFFER_TOO_SMALL;
    if (bins) *bins = w.nbins;
    return 0;
}

// v4 decoder (lep_dec4.h) as a 64-lane loop emulation
#include "../../lepton_amd/csrc/lep_dec4.h"
extern "C" int emu_decode_segment_v4(const lep_image_desc* d, int y0, int y1, int is_last, const uint8_t* in, uint32_t len, uint32_t* bins) {
    ImageDev img;
    int rc = derive_image(*d, &img, false);
    if (rc) return rc;
    std::vector<lep3::U4> model(lep3::kModelWords / 4, lep3::U4{kBranchInit, kBranchInit, kBranchInit, kBranchInit});
    std::vector<NSum> ns(img.ns_total);
    memset(ns.data(), 0, ns.size() * sizeof(NSum));
    SegDev seg;
    seg.image = 0; seg.y0 = y0; seg.y1 = y1; seg.is_last = is_last; seg.stream_off = 0; seg.stream_cap = 0;
    static lep4::Dec4Shared sh;
    lep4::Dec4Wave w;
    PaddedStream ps(in, len);
    rc = w.run(&img, seg, reinterpret_cast<uint32_t*>(model.data()), ns.data(), &sh, ps.p, len);
    if (bins) *bins = w.nbins;
    return rc;
}


// exhaustive check of the 24-bit table reciprocal used by lep4::bupd_t / bupd_u against Branch::record_obs_and_update
extern "C" int emu_check_inv24_update() {
    static uint32_t inv[512];
    for (uint32_t d = 0; d < 512; ++d) inv[d] = lep4::inv24_of(d);
    for (uint32_t f = 1; f < 256; ++f)
        for (uint32_t t = 1; t < 256; ++t) {
            if (inv[f + t] >= (1u << 24)) return 2;
            if ((lep4::mul24(f << 8, inv[f + t]) >> 24) != (f << 8) / (f + t)) return 3;
            for (uint32_t p = 0; p < 256; p += 51)
                for (uint32_t obs = 0; obs < 2; ++obs) {
                    uint32_t w = f | (t << 8) | (p << 16);
                    if (branch_update(w, (int)obs) != lep4::bupd_t(w, obs, inv)) return 4;
                    if (branch_update(w, (int)obs) != lep4::bupd_u(w, obs, inv)) return 5;
                }
        }
    return 0;
}

// lep4::div_by against `/`: every divisor the tables can hold (quantiser values 1..65535 as they are and times the eight
// ICOS column constants), numerators around the multiples of the divisor, the extremes and random ones
extern "C" int emu_check_div_by() {
    static const int32_t col0[9] = {1, 8192, 11363, 10703, 9633, 8192, 6436, 4433, 2260};
    uint64_t rnd = 0x9e3779b97f4a7c15ull;
    for (int c = 0; c < 9; ++c)
        for (uint32_t q = 1; q < 65536; ++q) {
            const int64_t d64 = (int64_t)col0[c] * q;
            if (d64 < 2 || d64 > 0x7fffffff) continue;
            const int32_t d = (int32_t)d64;
            const lep4::DivBy m = lep4::DivBy::of((uint32_t)d);
            int64_t ns[40];
            int k = 0;
            for (int64_t v : {(int64_t)0, (int64_t)1, (int64_t)-1, (int64_t)0x7fffffff, -(int64_t)0x80000000ll, (int64_t)d, (int64_t)d - 1, (int64_t)d + 1}) ns[k++] = v;
            for (int i = 0; i < 8; ++i) {
                rnd = rnd * 6364136223846793005ull + 1442695040888963407ull;
                const int64_t mult = (int64_t)((rnd >> 33) % (uint64_t)(0x7fffffff / d + 1));
                ns[k++] = mult * d; ns[k++] = mult * d - 1; ns[k++] = -(mult * d); ns[k++] = -(mult * d) + 1;
            }
            for (int i = 0; i < k; ++i) {
                if (ns[i] > 0x7fffffff || ns[i] < -(int64_t)0x80000000ll) continue;
                const int32_t n = (int32_t)ns[i];
                const int32_t want = (n == INT32_MIN && d == -1) ? 0 : (int32_t)((int64_t)n / d);
                if (lep4::div_by(n, m.mul, m.shift) != want) return 1 + c;
            }
        }
    return 0;
}

// GPU Huffman re-encoder (lep_huff.h) as a 64-lane loop emulation: scan bytes of one thread segment
#include "../../lepton_amd/csrc/lep_huff.h"
extern "C" int emu_huffman_encode_segment(const lep_huff_image* img, const lep_huff_segment* seg, uint8_t* out, uint32_t* len, lep_huff_end* end) {
    static lephuff::HuffShared sh;
    lephuff::HuffWave w;
    lephuff::HuffSegment s;
    memcpy(&s, seg, sizeof s);
    s.out_off = 0; s.image = 0;
    *len = w.run(reinterpret_cast<const lephuff::HuffImage*>(img), s, &sh, out);
    if (end) w.export_end(reinterpret_cast<lephuff::HuffEnd*>(end));
    return 0;
}

// ... with one lane per run of MCUs (lep_huff_simt.h): count, place, code, stuff for ONE segment; returns 1 when that form does not
// take the segment (restart intervals, ...), and then writes nothing
#include "../../lepton_amd/csrc/lep_huff_simt.h"
extern "C" int emu_huffman_encode_segment_simt(const lep_huff_image* img, const lep_huff_segment* seg, uint8_t* out, uint32_t* len, lep_huff_end* end) {
    static lephuff::SimtEncShared sh;
    const lephuff::HuffImage* im = reinterpret_cast<const lephuff::HuffImage*>(img);
    lephuff::HuffSegment s;
    memcpy(&s, seg, sizeof s);
    s.out_off = 0; s.image = 0;
    lephuff::SimtEncPlan plan;   // (the launch code's own: lep_gpu_huffman_encode_device)
    lephuff::simt_enc_plan(im, 1, &s, 1, true, &plan);
    if (plan.es.empty()) return 1;
    lephuff::SimtEncSeg es = plan.es[0];
    std::vector<uint32_t> unit_bits(es.nunits), unit_plain(es.nunits);
    std::vector<uint32_t> scratch(plan.scratch_bytes / 4 + 4, 0u);
    uint8_t* sc = reinterpret_cast<uint8_t*>(scratch.data());
    for (uint32_t f = 0; f < es.nunits; f += 64) lephuff::simt_enc_units<false>(im, &s, &es, &sh, unit_bits.data(), sc, f);
    lephuff::simt_enc_place(im, &s, &es, unit_bits.data(), unit_plain.data());
    for (uint32_t f = 0; f < es.nunits; f += 64) lephuff::simt_enc_units<true>(im, &s, &es, &sh, unit_bits.data(), sc, f);
    uint32_t n = 0;
    lephuff::simt_enc_stuff(im, &s, es, sc, out, &n, reinterpret_cast<lephuff::HuffEnd*>(end));
    *len = n;
    return 0;
}

// progressive scans (lep_huffprog.h): every scan of one image, one emulated wavefront after the other
#include "../../lepton_amd/csrc/lep_huffprog.h"
// (a scan of a SEQUENTIAL frame coded in several scans goes where the launch code sends it: to the sequential scan encoders, as an image with
// one segment -- lep_huffprog.h sequential_scan_segment, lep_gpu.hip lep_gpu_huffman_progressive_encode_device)
static uint32_t emu_sequential_scan(const lephuff::ProgImage* im, const lephuff::ProgScan& sc, uint8_t* out, bool lanes) {
    lephuff::HuffImage hi;
    lephuff::HuffSegment sg;
    lephuff::sequential_scan_segment(*im, sc, 0, &hi, &sg);
    uint32_t n = 0;
    lep_huff_end end;
    memset(&end, 0, sizeof end);
    int rc = 1;
    if (lanes) rc = emu_huffman_encode_segment_simt(reinterpret_cast<const lep_huff_image*>(&hi), reinterpret_cast<const lep_huff_segment*>(&sg), out + sc.out_off, &n, &end);
    if (rc == 1) emu_huffman_encode_segment(reinterpret_cast<const lep_huff_image*>(&hi), reinterpret_cast<const lep_huff_segment*>(&sg), out + sc.out_off, &n, &end);
    const bool over = end.attempted > sc.out_cap || (end.pad & (lephuff::kHuffEndCut | lephuff::kHuffEndRefused)) != 0;
    return n | (over ? 0x80000000u : 0u);
}
extern "C" int emu_huffman_progressive_encode(const lep_huffprog_image* img, const lep_huffprog_scan* scans, int nscan, uint8_t* out, uint32_t* corr, uint32_t* out_len) {
    static lephuff::ProgShared sh;
    for (int i = 0; i < nscan; ++i) {
        if (lephuff::prog_is_sequential(*reinterpret_cast<const lephuff::ProgScan*>(scans + i))) {
            out_len[i] = emu_sequential_scan(reinterpret_cast<const lephuff::ProgImage*>(img), *reinterpret_cast<const lephuff::ProgScan*>(scans + i), out, false);
            continue;
        }
        lephuff::ProgWave w;
        out_len[i] = w.run_scan(reinterpret_cast<const lephuff::ProgImage*>(img), reinterpret_cast<const lephuff::ProgScan*>(scans + i), &sh, out, corr);
    }
    return 0;
}

// ... with one lane per run of blocks (lep_huffprog_simt.h; prog_simt_driver.h steps the passes over the launch code's plan), scans with
// a restart interval left to the wavefront form.  taken[i]: 1 when the lane form -- or, for a scan of a sequential frame, the sequential
// scan encoders -- took scan i (the others are written by the wavefront form above, as on the GPU).
// region_bytes: > 0 stands in for the launch code's region size (tests: a region that does not suffice)
#include "prog_simt_driver.h"
extern "C" int emu_huffman_progressive_encode_simt(const lep_huffprog_image* img, const lep_huffprog_scan* scans, int nscan, uint8_t* out, uint32_t* corr, uint32_t* out_len,
                                                   int32_t* taken, uint64_t region_bytes) {
    int32_t intact = 0;
    const int rc = emu_prog_simt_drive(img, scans, nscan, out, corr, out_len, taken, region_bytes, false,
                                       [](const lephuff::ProgImage* im, const lephuff::ProgScan& sc, uint8_t* o) { return emu_sequential_scan(im, sc, o, true); }, &intact);
    return rc ? rc : (intact ? 0 : -1);   // (-1: a pass wrote outside the region or the unit arrays)
}

// GPU Huffman scan decoder (lep_huffdec.h) as a 64-lane loop emulation: one image
#include "../../lepton_amd/csrc/lep_huffdec.h"
extern "C" int emu_huffman_decode_image(const lep_huffdec_image* img, lep_huffdec_row* rows) {
    static lephuff::HuffDecShared sh;
    lephuff::HuffDecWave w;
    lephuff::HuffDecImage im;
    memcpy(&im, img, sizeof im);
    im.rows_off = 0;
    w.run(&im, &sh, reinterpret_cast<lephuff::HuffDecRow*>(rows));
    return 0;
}

// The scan decoders (lep_huffprogdec.h, _win.h, _rst.h; lep_huffdec_simt.h) as the launch code runs them: scan_dec_driver.h steps the passes
// over the launch code's own plans.  The entry points below say which knobs are on.
#include "scan_dec_driver.h"
static lephuff::ProgDecOptions emu_prog_dec_options(bool lanes, bool win, bool pipeline) {
    lephuff::ProgDecOptions o;
    o.lanes = lanes; o.win = win; o.rst = false; o.pipeline = pipeline; o.pipeline_max = 0x7fffffff; o.split = false;
    return o;
}
// progressive scans on lep_huffprogdec.h: the scans of one image, level by level (a scan of a SEQUENTIAL frame coded in several scans goes where
// the launch code sends it: to the sequential scan decoders, as an image of its own -- here the single-wave kernel)
extern "C" int emu_huffman_progressive_decode(const lep_huffprogdec_scan* scans, int nscan, lep_huffdec_row* rows) {
    return emu_prog_dec_drive(reinterpret_cast<const lephuff::ProgDecScan*>(scans), nscan, emu_prog_dec_options(false, false, false), reinterpret_cast<lephuff::HuffDecRow*>(rows));
}

// ... as ONE pipelined launch (all levels; a scan follows the scans of its file in front of it MCU row by MCU row): the launch
// order, the dependencies the plan works out (returned through deps_out[nscan][4], indices into the caller's array; none where the plan
// declines to pipeline -- one level, a scan that follows more than four) and the waiting / publishing code, run one scan after the other
// in launch order (a scan never finds the scans in front of it not far enough here; the code path that polls is the GPU's).
extern "C" int emu_huffman_progressive_decode_pipelined(const lep_huffprogdec_scan* scans, int nscan, lep_huffdec_row* rows, int32_t* deps_out) {
    return emu_prog_dec_drive(reinterpret_cast<const lephuff::ProgDecScan*>(scans), nscan, emu_prog_dec_options(false, false, true), reinterpret_cast<lephuff::HuffDecRow*>(rows), deps_out);
}

// ... with the window of speculative codes (lep_huffprogdec_win.h) for the scans that form takes: level by level (pipelined = 0) or
// in the one launch's order with its waiting / publishing code (pipelined = 1); sequential frames' scans one lane per subsequence where
// that decoder takes them.  taken: how many scans the window form decoded.
extern "C" int emu_huffman_progressive_decode_win(const lep_huffprogdec_scan* scans, int nscan, lep_huffdec_row* rows, int pipelined, int32_t* taken) {
    return emu_prog_dec_drive(reinterpret_cast<const lephuff::ProgDecScan*>(scans), nscan, emu_prog_dec_options(true, true, pipelined != 0), reinterpret_cast<lephuff::HuffDecRow*>(rows), nullptr, taken);
}

// one lane per subsequence (lep_huffdec_simt.h): guess, settle passes, place, write, finish -- every pass one wavefront after the other.
// settle_moved[k] (k = 0 .. kSimtSettle): whether pass k saw an end state move; nsub_out: subsequences the scan was cut into.
// side_array = false: a caller that passes no side array of slot sums (tests/test_blind_wide_emulation.py says what happens then).
static int emu_simt_decode_one(const lep_huffdec_image* img, lep_huffdec_row* rows, uint32_t sub_bits, int32_t* settle_moved, uint32_t* nsub_out, bool side_array) {
    lephuff::HuffDecImage im;
    memcpy(&im, img, sizeof im);
    im.rows_off = 0;
    if (!((sub_bits + 31u) & ~31u)) return -1;
    lephuff::SimtDecPlan plan;
    if (int rc = emu_simt_dec_drive(&im, 1, sub_bits, side_array, reinterpret_cast<lephuff::HuffDecRow*>(rows), &plan)) return rc;
    if (settle_moved) for (int k = 0; k <= lephuff::kSimtSettle; ++k) settle_moved[k] = plan.si[0].changed[k];
    if (nsub_out) *nsub_out = plan.si[0].nsub;
    return 0;
}
extern "C" int emu_huffman_decode_image_simt(const lep_huffdec_image* img, lep_huffdec_row* rows, uint32_t sub_bits, int32_t* settle_moved, uint32_t* nsub_out) {
    return emu_simt_decode_one(img, rows, sub_bits, settle_moved, nsub_out, false);
}

// split-phase encoder (lep_enc5.h): count -> plan -> emit -> fold (every chain) -> gather -> write, one segment, every pass
// stepped as a 64-lane loop emulation; bins_out (optional): the (probability | bit << 8) list the writer consumed
#include "../../lepton_amd/csrc/lep_enc5.h"
template <int NW>
static int encode_segment_v5(const lep_image_desc* d, int y0, int y1, int is_last, uint8_t* out, uint32_t cap, uint32_t* len, uint32_t* bins,
                             uint16_t* bins_out, uint32_t bins_out_cap, int nparts = 1) {
    using namespace lep5;
    ImageDev img;
    int rc = derive_image(*d, &img, true);
    if (rc) return rc;
    std::vector<NSum> ns(img.ns_total);
    SegDev seg;
    seg.image = 0; seg.y0 = y0; seg.y1 = y1; seg.is_last = is_last; seg.stream_off = 0; seg.stream_cap = cap; seg.slot = 0;
    static Walk5Shared wsh;
    static FoldShared fsh;
    std::vector<uint32_t> counts(kCountWords, 0);
    static SegPlan5 plan;
    {
        Walk5<kCount, NW> w;
        memset(ns.data(), 0, ns.size() * sizeof(NSum));
        w.run(&img, seg, ns.data(), &wsh, &plan, nullptr, nullptr);
        export_counts(w, &wsh, counts.data());
    }
    plan_segment(counts.data(), &plan);
    std::vector<uint8_t> arena(plan.arena_bytes + 64, 0xA5);   // poisoned: every byte read must have been written
    std::vector<uint16_t> binlist(plan.bins_cap + 64, 0xA5A5);
    {
        Walk5<kEmit, NW> w;
        memset(ns.data(), 0, ns.size() * sizeof(NSum));
        rc = w.run(&img, seg, ns.data(), &wsh, &plan, arena.data(), nullptr, 0, 0, nparts);
        if (rc) return rc;
        if (w.sign_pos[0] != plan.sign_cnt[0] || w.sign_pos[1] != plan.sign_cnt[1] || w.ord0 != plan.nblocks) return 1001;
        for (int i = 0; i < kStreams; ++i) if (wsh.cursor[i] != plan.base[i] + plan.cnt[i]) return 1002;
    }
    {
        static BucketShared bsh;
        bucket_wave(&plan, arena.data(), &bsh);
    }
    std::vector<uint32_t> thresh(kThreshWords, kBranchInit);
    for (int ci = 0; ci < 2; ++ci) {
        for (int row = 0; row < kRows; ++row)
            for (int k = 0; k < kClasses; ++k) {
                const int sid = stream_id(ci, row, k);
                if (!plan.cnt[sid]) continue;
                if (row < 63) fold_coef_wave(&plan, arena.data(), 0, 1, sid, &fsh);   // (row 63: the threshold chains of this colour index, class = lt)
                else fold_thresh_wave(&plan, arena.data(), thresh.data(), 0, 1, sid, ci, &fsh);
            }
        fold_sign_wave(&plan, arena.data(), 0, 1, ci, &fsh);
        for (int b = 0; b < 10; ++b) fold_nz_wave(&plan, arena.data(), 0, 1, ci, b, &fsh);
        for (int v = 0; v < 2; ++v) for (int e = 0; e < 8; ++e) fold_edgenz_wave(&plan, arena.data(), 0, 1, ci, v, e, &fsh);
    }
    for (int a = 0; a < 12; ++a) fold_dc_wave(&plan, arena.data(), 0, 1, a, &fsh);
    for (int part = 0; part < nparts; ++part) {   // (every part: a walker of its own, as on the GPU)
        Walk5<kGather, NW> w;
        memset(ns.data(), 0, ns.size() * sizeof(NSum));
        rc = w.run(&img, seg, ns.data(), &wsh, &plan, arena.data(), binlist.data(), 0, part, nparts);
        if (rc) return rc;
        if (w.nbins > plan.bins_cap) return 1003;
        if (part + 1 < nparts && w.nbins != reinterpret_cast<const Ckpt5*>(arena.data() + plan.ckpt_base)[part + 1].nbins) return 1004;   // emit's bin count at the checkpoint
        plan.nbins = w.nbins;
    }
    if (bins) *bins = plan.nbins;
    if (bins_out) memcpy(bins_out, binlist.data(), 2 * (size_t)(plan.nbins < bins_out_cap ? plan.nbins : bins_out_cap));
    uint32_t slen = 0;
    int32_t status = 0;
    for (int part = 0; part < nparts; ++part) write_wave(&plan, binlist.data(), &seg, 0, 1, out, &slen, &status, arena.data(), part, nparts);
    *len = slen;
    {   // the stitched writer over the same bin list (K chunks, K and the warm-up varied with the list): the same bytes, the same verdict
        const int K = 2 << (plan.nbins % 6);
        const uint32_t warms[4] = {kWarm5, 100, 3000, 1u << 22};
        std::vector<WChunk5> recs((size_t)K);
        memset(recs.data(), 0, recs.size() * sizeof(WChunk5));
        std::vector<uint8_t> again((size_t)cap + 64, 0x5A);
        uint32_t slen2 = 0;
        int32_t status2 = 0;
        for (int k = 0; k < K; ++k) wchunk_range_lane(plan, binlist.data(), &recs[(size_t)k], k, K, warms[(plan.nbins >> 3) & 3]);
        wchunk_link_lane(plan, binlist.data(), recs.data(), K);
        for (int k = 0; k < K; ++k) wchunk_code_lane(plan, binlist.data(), seg, again.data(), &recs[(size_t)k], k, K);
        wchunk_stitch_lane(plan, seg, again.data(), &slen2, &status2, recs.data(), K);
        if ((status2 == 100) != (status == 100)) return 1006;
        if (status != 100 && (slen2 != slen || memcmp(again.data(), out, slen))) return 1007;
    }
    return status == 100 ? LEP_BUFFER_TOO_SMALL : status;
}
extern "C" int emu_encode_segment_v5(const lep_image_desc* d, int y0, int y1, int is_last, uint8_t* out, uint32_t cap, uint32_t* len, uint32_t* bins,
                                     uint16_t* bins_out, uint32_t bins_out_cap) {
    return encode_segment_v5<1>(d, y0, y1, is_last, out, cap, len, bins, bins_out, bins_out_cap);
}
// ... with the walks split into their two halves (what two wavefronts per segment run side by side on the GPU)
extern "C" int emu_encode_segment_v5_halves(const lep_image_desc* d, int y0, int y1, int is_last, uint8_t* out, uint32_t cap, uint32_t* len, uint32_t* bins,
                                            uint16_t* bins_out, uint32_t bins_out_cap) {
    return encode_segment_v5<2>(d, y0, y1, is_last, out, cap, len, bins, bins_out, bins_out_cap);
}
// ... with gather and write in parts (tile ranges of the segment, taken up from emit's checkpoints; the writer's state carried over)
extern "C" int emu_encode_segment_v5_parts(const lep_image_desc* d, int y0, int y1, int is_last, uint8_t* out, uint32_t cap, uint32_t* len, uint32_t* bins,
                                           uint16_t* bins_out, uint32_t bins_out_cap) {
    const int rc = encode_segment_v5<2>(d, y0, y1, is_last, out, cap, len, bins, bins_out, bins_out_cap, 4);
    if (rc) return rc;
    std::vector<uint8_t> again(cap);
    uint32_t len2 = 0, bins2 = 0;
    const int rc2 = encode_segment_v5<1>(d, y0, y1, is_last, again.data(), cap, &len2, &bins2, nullptr, 0, 7);   // one wavefront, seven parts: the same bytes
    if (rc2) return rc2;
    return (len2 == *len && !memcmp(again.data(), out, len2)) ? 0 : 1005;
}


// lep5::BoolEnc5 (deferred byte output, carry cache) against the serial writer of lep_core.h on random and adversarial bin
// sequences: uniform, nearly-certain bins coded wrong (long shifts), runs that produce 0xFF bytes and carries into them, tiny
// output buffers (overflow verdicts).  Returns 0, or 1 + the trial that differed.
extern "C" int emu_check_bool_writer5(int trials) {
    uint64_t rs = 88172645463325252ull;
    auto rnd = [&]() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t)(rs >> 11); };
    std::vector<uint8_t> a(1 << 16), b(1 << 16);
    for (int trial = 0; trial < trials; ++trial) {
        const int n = (int)(rnd() % 3000), mode = trial % 6;
        std::vector<uint16_t> bins((size_t)n);
        for (int i = 0; i < n; ++i) {
            uint32_t p, bit;
            if (mode == 0) { p = rnd() % 256; bit = rnd() & 1; }
            else if (mode == 1) { p = 1 + rnd() % 3; bit = (rnd() % 8) != 0; }
            else if (mode == 2) { p = 250 + rnd() % 6; bit = (rnd() % 8) == 0; }
            else if (mode == 3) { p = 128; bit = 1; }
            else if (mode == 4) { p = rnd() % 256; bit = (rnd() % 256) < p ? 0 : 1; }
            else { p = (rnd() & 1) ? 255 : 1; bit = rnd() & 1; }
            bins[(size_t)i] = (uint16_t)(p | (bit << 8));
        }
        const uint32_t cap = (trial % 50 == 0) ? rnd() % 200 : 1u << 16;
        memset(a.data(), 0xAA, a.size()); memset(b.data(), 0xBB, b.size());
        lepdev::BoolCoder<false> ref;
        ref.init_stream(a.data(), cap);
        for (int i = 0; i < n; ++i) ref.put(bins[(size_t)i] >> 8, bins[(size_t)i] & 255);
        const uint32_t la = ref.finish();
        lep5::BoolEnc5 e;
        e.init(b.data(), cap);
        e.bin(0, 128);
        int g = 1;
        for (int i = 0; i < n; ++i) { e.bin(bins[(size_t)i] >> 8, bins[(size_t)i] & 255); if (++g == 4) { e.flush(); g = 0; } }
        bool ov = false;
        const uint32_t lb = e.finish(&ov);
        if (ref.overflow != ov) return 1 + trial;
        if (!ov && (la != lb || memcmp(a.data(), b.data(), la))) return 1 + trial;
    }
    return 0;
}


// the stitched writer (lep_enc5.h: range / link / code / stitch over K chunks of a bin list) against lepdev::BoolCoder<false>: bin
// lists of up to 40,000 bins in the six flavours above, K = 2 .. 64, warm-ups from 8 bins (every guess wrong: the link pass redoes
// the chunks) to longer than the list (every chunk warmed up from the stream's start), tiny buffers.  Returns 0 or 1 + the trial;
// *redone counts the chunks whose guessed start range was wrong.
extern "C" int emu_check_stitched_writer5(int trials, int* redone) {
    uint64_t rs = 0x2545F4914F6CDD1Dull;
    auto rnd = [&]() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t)(rs >> 11); };
    std::vector<uint8_t> a(1 << 17), b(1 << 17);
    int wrong = 0;
    for (int trial = 0; trial < trials; ++trial) {
        const int n = (int)(rnd() % (trial % 7 == 0 ? 40000 : 3000)), mode = trial % 6;
        std::vector<uint16_t> bins((size_t)n + 256, 0);
        for (int i = 0; i < n; ++i) {
            uint32_t p, bit;
            if (mode == 0) { p = rnd() % 256; bit = rnd() & 1; }
            else if (mode == 1) { p = 1 + rnd() % 3; bit = (rnd() % 8) != 0; }
            else if (mode == 2) { p = 250 + rnd() % 6; bit = (rnd() % 8) == 0; }
            else if (mode == 3) { p = 128; bit = 1; }
            else if (mode == 4) { p = rnd() % 256; bit = (rnd() % 256) < p ? 0 : 1; }
            else { p = (rnd() & 1) ? 255 : 1; bit = rnd() & 1; }
            bins[(size_t)i] = (uint16_t)(p | (bit << 8));
        }
        const uint32_t cap = (trial % 50 == 0) ? rnd() % 200 : 1u << 17;
        memset(a.data(), 0xAA, a.size()); memset(b.data(), 0xBB, b.size());
        lepdev::BoolCoder<false> ref;
        ref.init_stream(a.data(), cap);
        for (int i = 0; i < n; ++i) ref.put(bins[(size_t)i] >> 8, bins[(size_t)i] & 255);
        const uint32_t la = ref.finish();
        const int K = 2 << (rnd() % 6);
        const uint32_t warms[5] = {8, 64, 700, 16384, 1u << 20};
        const uint32_t warm = warms[rnd() % 5];
        lep5::SegPlan5 P;
        memset(&P, 0, sizeof P);
        P.nbins = (uint32_t)n; P.bins_off = 0; P.status = 0;
        SegDev sd;
        memset(&sd, 0, sizeof sd);
        sd.stream_off = 0; sd.stream_cap = cap; sd.slot = 0;
        std::vector<lep5::WChunk5> recs((size_t)K);
        memset(recs.data(), 0, recs.size() * sizeof(lep5::WChunk5));
        for (int k = 0; k < K; ++k) lep5::wchunk_range_lane(P, bins.data(), &recs[(size_t)k], k, K, warm);
        for (int k = 1; k < K; ++k) wrong += recs[(size_t)k].q_guess != recs[(size_t)k - 1].q_end;   // (before link: against the unlinked ends -- an upper bound)
        lep5::wchunk_link_lane(P, bins.data(), recs.data(), K);
        for (int k = K - 1; k >= 0; --k) lep5::wchunk_code_lane(P, bins.data(), sd, b.data(), &recs[(size_t)k], k, K);   // any order: the chunks do not meet
        uint32_t lb = 0;
        int32_t stt = 0;
        lep5::wchunk_stitch_lane(P, sd, b.data(), &lb, &stt, recs.data(), K);
        const bool ov = stt == 100;
        if (ref.overflow != ov) return 1 + trial;
        if (!ov && (la != lb || memcmp(a.data(), b.data(), la))) return 1 + trial;
    }
    if (redone) *redone = wrong;
    return 0;
}

// the 16-bit Branch of the fold lanes (lep5::upd16 / prob16) against the packed word of lep_core.h (branch_update): random walks
// with every bias, long enough to saturate either way and to renormalise; returns 0 or 1 + the walk that differed
extern "C" int emu_check_branch16(int walks) {
    uint64_t rs = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t)(rs >> 11); };
    for (int w = 0; w < walks; ++w) {
        uint32_t a = lepdev::kBranchInit, b = lep5::kBranchInit16;
        const uint32_t bias = (w % 9) * 32;   // 0: always false ... 256: always true
        for (int i = 0; i < 3000; ++i) {
            if (lep5::prob16(b) != (a >> 16)) return 1 + w;
            uint32_t obs = (rnd() % 256) < bias ? 1u : 0u;
            if (w % 7 == 3 && i > 300 && i < 310) obs ^= 1u;   // a few surprises after saturation
            a = lepdev::branch_update(a, (int)obs);
            b = lep5::upd16(b, obs);
        }
    }
    return 0;
}

// the count walk's result for one segment: counts[lep5::kCountWords] (units per stream, sign bytes, blocks, bins bound, tiles)
extern "C" int emu_v5_counts(const lep_image_desc* d, int y0, int y1, int is_last, uint32_t* counts) {
    using namespace lep5;
    ImageDev img;
    int rc = derive_image(*d, &img, true);
    if (rc) return rc;
    std::vector<NSum> ns(img.ns_total);
    SegDev seg;
    seg.image = 0; seg.y0 = y0; seg.y1 = y1; seg.is_last = is_last; seg.stream_off = 0; seg.stream_cap = 0; seg.slot = 0;
    static Walk5Shared wsh;
    static SegPlan5 plan;
    Walk5<kCount> w;
    memset(ns.data(), 0, ns.size() * sizeof(NSum));
    w.run(&img, seg, ns.data(), &wsh, &plan, nullptr, nullptr);
    export_counts(w, &wsh, counts);
    return 0;
}

// lep_huffprogdec.h prog_scan_deps on descriptors a test made up (only the frame pointer, the components and the band are looked at)
extern "C" int emu_prog_scan_deps(const lep_huffprogdec_scan* scans, const int* order, int n, int32_t* deps_out) {
    std::vector<lephuff::ProgDeps> deps((size_t)n);
    const bool ok = lephuff::prog_scan_deps(reinterpret_cast<const lephuff::ProgDecScan*>(scans), order, n, deps.data());
    for (int i = 0; i < n; ++i) for (int d = 0; d < 4; ++d) deps_out[4 * i + d] = deps[(size_t)i].dep[d];
    return ok ? 1 : 0;
}

// one bin list (probability | bit << 8) through lepdev::BoolCoder<false> into `cap` bytes of room: start marker, bins, 32 stop bins, end
// rule; the reference tests/bool_writer_ref.py is held against it
extern "C" int emu_bool_writer_list(const uint16_t* bins, uint32_t n, uint8_t* out, uint32_t cap, uint32_t* len, int* overflow) {
    lepdev::BoolCoder<false> ref;
    ref.init_stream(out, cap);
    for (uint32_t i = 0; i < n; ++i) ref.put(bins[i] >> 8, bins[i] & 255);
    *len = ref.finish();
    *overflow = ref.overflow ? 1 : 0;
    return 0;
}

// ... and through the split-phase encoder's writer as lep_gpu_debug_write_bins launches it on the GPU (form 0 write_wave in `parts` parts,
// 1 the stitched writer over `chunks` chunks, 2 `chunks` chunks per part, part by part; part_first[parts] the parts' first bins, kWarm5):
// bytes, length, status and, for the chunked forms, the records (parts * chunks of them).  The list has room to the next multiple of
// 128 bins and 256 bytes behind, the later parts' bins are 0xA5A5 until their part comes, nbins is there from the last part on.
extern "C" int emu_write_bins5(int form, int parts, int chunks, const uint16_t* bins, uint32_t n, const uint32_t* part_first, int plan_status,
                               uint8_t* out, uint32_t cap, uint32_t* len, int32_t* status, lep5::WChunk5* recs) {
    using namespace lep5;
    if (parts < 1 || parts > kMaxParts || chunks < 1) return 1;
    std::vector<uint16_t> work(((size_t)n + 127) / 128 * 128 + 128, 0xA5A5);
    std::vector<uint8_t> arena(1024, 0xEE);
    SegPlan5 plan;
    memset(&plan, 0, sizeof plan);
    plan.ckpt_base = 0; plan.wstate_base = (uint32_t)(kMaxParts * sizeof(Ckpt5)); plan.status = plan_status;
    Ckpt5* ck = reinterpret_cast<Ckpt5*>(arena.data());
    uint32_t B[kMaxParts + 1];
    for (int p = 0; p < parts; ++p) B[p] = p == 0 ? 0u : part_first[p];
    B[parts] = n;
    for (int p = 1; p < parts; ++p) ck[p].nbins = B[p];
    SegDev sd;
    memset(&sd, 0, sizeof sd);
    sd.stream_cap = cap;
    *len = 0x7f7f7f7fu; *status = 0;   // (the kernels clear the status before the writer runs)
    if (form == 1) {
        memcpy(work.data(), bins, (size_t)n * 2);
        plan.nbins = n;
        for (int k = 0; k < chunks; ++k) wchunk_range_lane(plan, work.data(), recs + k, k, chunks);
        wchunk_link_lane(plan, work.data(), recs, chunks);
        for (int k = 0; k < chunks; ++k) wchunk_code_lane(plan, work.data(), sd, out, recs + k, k, chunks);
        wchunk_stitch_lane(plan, sd, out, len, status, recs, chunks);
        return 0;
    }
    plan.nbins = parts > 1 ? 0xEEEEEEEEu : n;
    for (int p = 0; p < parts; ++p) {
        for (uint32_t i = B[p]; i < B[p + 1]; ++i) work[i] = bins[i];
        if (p + 1 == parts) plan.nbins = n;
        if (form == 0) { write_wave(&plan, work.data(), &sd, 0, 1, out, len, status, arena.data(), p, parts); continue; }
        const int c = chunks;
        for (int s = 0; s < c; ++s) wchunk_range_cut(plan, work.data(), recs + p * c + s, part_chunk_cut(plan, ck, p, s, parts, c));
        wchunk_link_cuts(plan, work.data(), recs, p * c, (p + 1) * c, [&](int j) { return part_chunk_cut(plan, ck, j / c, j % c, parts, c); });
        for (int s = 0; s < c; ++s) wchunk_code_cut(plan, work.data(), sd, out, recs + p * c + s, part_chunk_cut(plan, ck, p, s, parts, c));
    }
    if (form == 2) wchunk_stitch_lane(plan, sd, out, len, status, recs, parts * chunks);
    return 0;
}
